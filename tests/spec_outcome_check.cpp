// Host check of spec_outcome (mh-spgemm_amd/csrc/mhs_shape.hpp): what becomes of a call after the
// hand-off, as a function of (spec, launched, err, same).  A stand-alone program, built with
// -fsanitize=address,undefined by tests/test_spec_outcome_host.py.  The 16 expected outcomes below are
// literals written out from the table in DESIGN.md (launch plan speculation); none comes from the
// function under test.
//
// The expression this function replaced,
//     !launched ? proceed : !err && same ? hit : err ? proceed (report the error) : rerun,
// gets these rows wrong (marked "was PROCEED" below):
//   (spec, !launched, !same): no room for the plan's C while the pattern changed in place -- C was
//       sized and filled from Stats whose left-out symbolic bins held stale counts;
//   (spec, err), launched or not: an error bit of a speculated call was reported as the call's result,
//       though k_scan may have summed stale counts past INT32_MAX (a false overflow).
#include "../mh-spgemm_amd/csrc/mhs_shape.hpp"

#include <cstdio>

using namespace mhs;

struct Row {
    bool spec, launched, err, same;
    SpecOutcome want;
};

static const Row TABLE[16] = {
    // a call that did not speculate: the ordinary numeric phase, an error reported from its own Stats
    {false, false, false, false, SPEC_PROCEED},
    {false, false, false, true, SPEC_PROCEED},
    {false, false, true, false, SPEC_PROCEED},
    {false, false, true, true, SPEC_PROCEED},
    {false, true, false, false, SPEC_PROCEED},
    {false, true, false, true, SPEC_PROCEED},
    {false, true, true, false, SPEC_PROCEED},
    {false, true, true, true, SPEC_PROCEED},
    // speculated, phase A stayed in (no room for the plan's C)
    {true, false, false, false, SPEC_RERUN},   // was PROCEED
    {true, false, false, true, SPEC_PROCEED},  // nothing was left out that the plan did not also leave out
    {true, false, true, false, SPEC_RERUN},    // was PROCEED
    {true, false, true, true, SPEC_RERUN},     // was PROCEED
    // speculated, phase A went out
    {true, true, false, false, SPEC_RERUN},
    {true, true, false, true, SPEC_HIT},
    {true, true, true, false, SPEC_RERUN},  // was PROCEED
    {true, true, true, true, SPEC_RERUN},   // was PROCEED
};

// the table covers every combination once
static_assert(SPEC_PROCEED != SPEC_HIT && SPEC_HIT != SPEC_RERUN && SPEC_PROCEED != SPEC_RERUN, "three outcomes");
static_assert(spec_outcome(true, true, false, true) == SPEC_HIT, "usable in constant expressions");

int main() {
    int failures = 0, seen = 0;
    for (const Row& r : TABLE) {
        const int idx = r.spec * 8 + r.launched * 4 + r.err * 2 + r.same;
        if (seen & (1 << idx)) {
            ++failures;
            fprintf(stderr, "combination %d listed twice\n", idx);
        }
        seen |= 1 << idx;
        const SpecOutcome got = spec_outcome(r.spec, r.launched, r.err, r.same);
        if (got != r.want) {
            ++failures;
            fprintf(stderr, "spec %d launched %d err %d same %d: outcome %d, expected %d\n", r.spec, r.launched, r.err,
                    r.same, (int)got, (int)r.want);
        }
    }
    if (seen != 0xFFFF) {
        ++failures;
        fprintf(stderr, "combinations covered: %#x\n", seen);
    }
    // only a speculated call can hit or rerun, and a rerun (spec false) therefore cannot rerun again
    int hits = 0, reruns = 0;
    for (int i = 0; i < 16; ++i) {
        const SpecOutcome o = spec_outcome(i & 8, i & 4, i & 2, i & 1);
        hits += o == SPEC_HIT;
        reruns += o == SPEC_RERUN;
    }
    if (hits != 1 || reruns != 6) {
        ++failures;
        fprintf(stderr, "hits %d reruns %d, expected 1 and 6\n", hits, reruns);
    }
    if (failures) return 1;
    printf("spec outcome ok\n");
    return 0;
}
