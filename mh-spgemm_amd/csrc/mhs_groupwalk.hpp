// mhs_groupwalk.hpp -- the take rule of the grouped numeric bins' cursor walk, host and device.
//
// A grouped launch (k_num_wave<.., grouped>) of about the resident set of waves walks its bin's
// list of group heads in eighths: XCD group g = blockIdx % 8 owns the g-th eighth of the list.
// Its waves (wave j of the group: block blockIdx / 8, wave w: j = blockIdx / 8 * WPB + w) stride
// through the eighth's first rounds statically -- round s gives wave j the index begin + s * waves
// + j -- and draw the rest, the last GROUP_DYN_ROUNDS full rounds and the partial one, as tickets
// 0, 1, 2, ... from the group's row cursor, one atomic each: ticket t is list index split + t
// while that lies in the eighth, every later ticket is "none": the eighth is done, the wave stops
// drawing.  (Every group from the cursor measured slower than the static grid: a ticket is a
// device-scope atomic, and the waves of a round ask for theirs at the same time.)
// A wave draws its next ticket while it still works on a group, so at its end it holds one ticket
// it may never use -- that one is always a "none" (it stops only on a "none"), and no list entry
// is read for it.  Nothing here depends on which waves are resident: no wave waits for another, a
// block that starts after the eighth is spent walks its static rounds, draws a "none" and returns.
// No HIP in it (mhs_shape.hpp's decorators are empty for a host compiler):
// tests/group_walk_check.cpp runs the rule on the host.
#pragma once
#include "mhs_shape.hpp"

namespace mhs {

constexpr int GROUP_NONE = -1;
constexpr int GROUP_XCDS = 8;  // cursors of a slot (CURSOR_STRIDE ints apart), eighths of a list
#ifndef MHS_GROUP_DYN_ROUNDS
#define MHS_GROUP_DYN_ROUNDS 1
#endif
constexpr int GROUP_DYN_ROUNDS = MHS_GROUP_DYN_ROUNDS;  // full rounds of an eighth left to the cursor

// XCD group g's eighth of a list of `count` entries: [group_begin(count, g), group_begin(count, g + 1))
__host__ __device__ inline int group_begin(int count, int g) { return (int)((long long)count * g / GROUP_XCDS); }

// The walk of XCD group g in a launch of `blocks` blocks (a multiple of 8) over `count` entries.
struct GroupWalk {
    int begin, split, end;  // the eighth [begin, end): [begin, split) in static rounds, [split, end) by ticket
    int waves;              // waves of the group: the static rounds' stride
};
__host__ __device__ inline GroupWalk group_walk(int count, int g, int blocks) {
    GroupWalk w;
    w.begin = group_begin(count, g);
    w.end = group_begin(count, g + 1);
    w.waves = blocks / GROUP_XCDS * WPB;
    const int rounds = w.waves > 0 ? (w.end - w.begin) / w.waves : 0;
    w.split = w.begin + (rounds > GROUP_DYN_ROUNDS ? rounds - GROUP_DYN_ROUNDS : 0) * w.waves;
    return w;
}
// Wave j's first index of the static rounds (GROUP_NONE: it has none), and the one after `li`.
__host__ __device__ inline int group_static_first(const GroupWalk& w, int j) {
    return w.begin + j < w.split ? w.begin + j : GROUP_NONE;
}
__host__ __device__ inline int group_static_next(const GroupWalk& w, int li) {
    return li + w.waves < w.split ? li + w.waves : GROUP_NONE;
}
// The list index of ticket `ticket` (>= 0, the value the cursor's atomic add returned), or
// GROUP_NONE past the eighth's end.
__host__ __device__ inline int group_take(const GroupWalk& w, int ticket) {
    return (unsigned)ticket < (unsigned)(w.end - w.split) ? w.split + ticket : GROUP_NONE;
}

// Blocks of the resident set of a grouped launch: per CU as many blocks of WPB waves as the
// kernel's 4 waves per SIMD (4 blocks) and the CU's LDS (regions of wave_bytes) allow.
__host__ __device__ inline int group_resident_blocks(int cus, int wave_bytes) {
    const int by_lds = wave_bytes > 0 ? LDS_MAX_C / (WPB * wave_bytes) : 4;
    const int per_cu = by_lds < 4 ? (by_lds < 1 ? 1 : by_lds) : 4;
    return cus * per_cu;
}

}  // namespace mhs
