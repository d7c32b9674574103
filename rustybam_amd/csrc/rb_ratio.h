// rb_ratio.h -- the three identities of a stats line, stated once for every kernel that writes them (k_records.hip, k_hitstats.hip,
// k_alnstats.hip).  bamstats.rs:138-142: (100.0 * equal as f32) / (u32 sum) as f32 -- the product first, then a correctly rounded
// divide, no contraction (the Makefile builds with -ffp-contract=off).  A sum of 0 gives NaN (0 / 0), as the reference prints it.
#pragma once
#include <stdint.h>

template <typename Row>
__device__ __forceinline__ void rb_identity_ratios(Row &w) { // reads equal, diff, ins, del, ins_events, del_events (u32) of the row
    const float num = 100.0f * (float)w.equal;
    w.id_by_all = num / (float)(uint32_t)(w.equal + w.diff + w.del + w.ins);
    w.id_by_events = num / (float)(uint32_t)(w.equal + w.diff + w.del_events + w.ins_events);
    w.id_by_matches = num / (float)(uint32_t)(w.equal + w.diff);
}
