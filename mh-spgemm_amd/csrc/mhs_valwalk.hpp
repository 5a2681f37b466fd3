// mhs_valwalk.hpp -- device helpers shared by the values kernels (mhs_values.hip) and their
// backward (mhs_values_grad.hip): the wave-level LDS ordering point, the slot search, and the
// stage of A entries that the wave and block walks read their B rows from.
#pragma once
#include "mhs_internal.hpp"

namespace mhs {

// Ordering point for LDS traffic between lanes of one wave (a wave's LDS operations are
// performed in issue order; only the compiler must not move accesses across it).
static __device__ __forceinline__ void vwave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Position of column c in the ascending cols[0, n), or -1.
static __device__ __forceinline__ int find_slot(const int* cols, int n, int c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cols[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && cols[lo] == c ? lo : -1;
}

// Up to CH staged A entries of a row as (B row start, length, A value); entry e of the stage that
// began at A position k0 is A entry k0 + e.
template <int CH>
struct ValStage {
    int bs[CH], len[CH];
    double av[CH];
};
constexpr int VAL_PIECES = 8;  // G-wide pieces of a B row a lane group loads before its first sum

}  // namespace mhs
