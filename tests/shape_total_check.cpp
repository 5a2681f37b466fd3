// shape_total_check.cpp -- the row classification of csrc/mhs_shape.hpp ends on any ints.
//
// k_scan classifies every row of a call before it gives its verdict on a speculated plan, also the rows of
// symbolic launches the call left out, whose tile and entry counts are whatever their words held (a freshly
// allocated workspace, a recycled C.ptr: tests/test_gpu_poison.py).  The class of such a row means nothing and the
// verdict is a miss, but every function on the way has to return: this program calls them on every combination of
// a few hostile ints and prints a checksum.  (next_pow2 once looped for ever above 2^30.)  Built without
// sanitizers: sums of garbage overflow by design.
//
//   c++ -std=c++17 -O0 -Wall -Werror -I mh-spgemm_amd/csrc tests/shape_total_check.cpp -o shape_total_check
#include <climits>
#include <cstdio>
#include <initializer_list>

#include "mhs_shape.hpp"

using namespace mhs;

int main() {
    const int hostile[] = {INT_MIN, -1, 0, 1, 193, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 0x7f7f7f7f, INT_MAX};
    long long sum = 0, calls = 0;
    for (int x : hostile) sum += next_pow2(x) + hash_sort_p(x) + hash_slots(x) + hash_slots_pow2(x);
    for (int span : hostile)
        for (int t : hostile)
            for (int n : hostile)
                for (int dense : {0, 4}) {
                    sum += num_mode(span, t, n, dense) + num_need(span, t, n, dense) + num_need_rows(span, t, n, dense, 3);
                    sum += num_wide(span, t, n, dense) + 2 * num_ranked(span, t, n, dense) + num_need_ranked(span, t, n);
                    sum += sym_direct(span, t) + sym_need(span, t) + mcached(span, t) + mlisted(span, t, n, MC_LIST_MAX);
                    sum += tiny_class(n, t) + tiny_class_sym(n, t);
                    ++calls;
                }
    std::printf("%lld calls, checksum %lld\n", calls, sum);
    return 0;
}
