// mhs_owner.hpp -- scope-bound owner of the device arrays a call builds its C in.
//
// A call that returns MHS_OK commits: the caller's mhs_csr is written and the owner holds
// nothing.  Every other way out of the scope gives the arrays back: the streams the call has
// queued work on are synchronised first (when anything was queued), then ptr, col and val
// are released and nulled.  The two deliberate hand-backs of a call that goes on -- a
// speculation miss, the switch to the row-chunked path -- are explicit give_back calls; they
// do not synchronise (their callers have, or are about to).
//
// No HIP here: Ops supplies  static void release(Ctx*, void*, bool pooled)  (pooled: into the
// context's caching pool, else a real free; a null pointer is a no-op) and
// static void sync(Ctx*)  (results ignored).  tests/owner_check.cpp runs it on the host.
#pragma once
#include "../../include/mhspgemm.h"

namespace mhs {

template <class Ctx, class Ops>
struct OutputOwner {
    mhs_csr out{};
    Ctx* ctx;
    bool pooled;          // release mode: the context's pool (mhs_spgemm) or a real free (row-chunked C)
    // device work referencing the arrays is, or is about to be, queued: set by the call when it
    // hands the first array to its launches (a wait too many on an early error exit is harmless)
    bool queued = false;

    OutputOwner(Ctx* c, bool pool) : ctx(c), pooled(pool) {}
    OutputOwner(const OutputOwner&) = delete;
    OutputOwner& operator=(const OutputOwner&) = delete;
    ~OutputOwner() {
        if (!out.ptr && !out.col && !out.val) return;
        if (queued) Ops::sync(ctx);
        give_back();
    }

    // the call succeeded: C is the caller's
    void commit(mhs_csr* C) {
        *C = out;
        out.ptr = nullptr;
        out.col = nullptr;
        out.val = nullptr;
    }
    // col / val back (ptr kept)
    void give_back_cols() {
        Ops::release(ctx, out.col, pooled);
        Ops::release(ctx, out.val, pooled);
        out.col = nullptr;
        out.val = nullptr;
    }
    void give_back() {
        Ops::release(ctx, out.ptr, pooled);
        out.ptr = nullptr;
        give_back_cols();
    }
};

}  // namespace mhs
