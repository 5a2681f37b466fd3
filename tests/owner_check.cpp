// Host check of OutputOwner (mh-spgemm_amd/csrc/mhs_owner.hpp), the scope-bound owner of a
// call's C arrays: a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_host.py.  The "device arrays" are heap blocks, so a leak, a double release or a
// release of a committed array is the sanitizer's finding as well as a failed count below.
#include "../mh-spgemm_amd/csrc/mhs_owner.hpp"

#include <cstdio>
#include <cstdlib>

struct Ctx {
    int pooled = 0, freed = 0, syncs = 0;
    int syncs_at_first_release = -1;
};

struct Ops {
    static void release(Ctx* c, void* p, bool pooled) {
        if (!p) return;
        if (c->syncs_at_first_release < 0) c->syncs_at_first_release = c->syncs;
        ++(pooled ? c->pooled : c->freed);
        free(p);
    }
    static void sync(Ctx* c) { ++c->syncs; }
};
using Owner = mhs::OutputOwner<Ctx, Ops>;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            ++failures;                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
        }                                                               \
    } while (0)

static void fill(Owner& o, bool cols = true) {
    o.out.ptr = (int32_t*)malloc(16);
    if (cols) o.out.col = (int32_t*)malloc(16);
    if (cols) o.out.val = (double*)malloc(16);
}

int main() {
    {  // commit: the caller has the arrays, nothing is released or waited for
        Ctx c;
        mhs_csr C{};
        {
            Owner o(&c, true);
            fill(o);
            o.out.nnz = 4;
            o.queued = true;
            o.commit(&C);
            CHECK(!o.out.ptr && !o.out.col && !o.out.val);
        }
        CHECK(c.pooled == 0 && c.freed == 0 && c.syncs == 0);
        CHECK(C.ptr && C.col && C.val && C.nnz == 4);
        free(C.ptr), free(C.col), free(C.val);
    }
    {  // early exit, nothing queued: released to the pool without a wait
        Ctx c;
        {
            Owner o(&c, true);
            fill(o, false);
        }
        CHECK(c.pooled == 1 && c.freed == 0 && c.syncs == 0);
    }
    {  // early exit with queued work: one wait, before the first release
        Ctx c;
        {
            Owner o(&c, true);
            fill(o);
            o.queued = true;
        }
        CHECK(c.pooled == 3 && c.syncs == 1 && c.syncs_at_first_release == 1);
    }
    {  // the free mode (row-chunked C)
        Ctx c;
        {
            Owner o(&c, false);
            fill(o);
            o.queued = true;
        }
        CHECK(c.freed == 3 && c.pooled == 0 && c.syncs == 1);
    }
    {  // speculation miss: col / val back and ptr kept, then ptr too; the scope's end finds nothing
        Ctx c;
        {
            Owner o(&c, true);
            fill(o);
            o.queued = true;
            o.give_back_cols();
            CHECK(c.pooled == 2 && o.out.ptr && !o.out.col && !o.out.val);
            o.give_back();
            CHECK(c.pooled == 3 && !o.out.ptr);
        }
        CHECK(c.pooled == 3 && c.syncs == 0);
    }
    {  // miss with ptr kept (the call goes on to report an error): the exit gives it back
        Ctx c;
        {
            Owner o(&c, true);
            fill(o);
            o.queued = true;
            o.give_back_cols();
        }
        CHECK(c.pooled == 3 && c.syncs == 1);
    }
    {  // double release
        Ctx c;
        {
            Owner o(&c, true);
            fill(o);
            o.give_back();
            o.give_back();
            o.give_back_cols();
        }
        CHECK(c.pooled == 3 && c.syncs == 0);
    }
    {  // an empty owner (allocation never happened)
        Ctx c;
        {
            Owner o(&c, true);
            o.queued = true;
        }
        CHECK(c.pooled == 0 && c.syncs == 0);
    }
    if (failures) return 1;
    puts("owner ok");
    return 0;
}
