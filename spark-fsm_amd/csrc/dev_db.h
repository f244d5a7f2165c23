// dev_db.h — the flattened DBs resident in HBM (built by fsm_db_from_*: the
// host flatten + upload, or K0 on the device, k0_build.hip).
#pragma once

#include <vector>

#include "fsm_internal.h"

// SPADE: one row per distinct sequence id; each row holds its distinct items
// (ascending dense id) with the W-word mask of their rank-compressed eids.
struct SpadeDevDB {
    fsm::DevBuf row_off;  // u32 [R+1]
    fsm::DevBuf item;     // u32 [E]
    fsm::DevBuf mask;     // u64 [E*W]
    int64_t R = 0, E = 0, U = 0;
    int W = 1;
    // F1 (spade_engine.hip, k_f1): every item's distinct-sequence support, a property of the DB,
    // kept by the handle's first unsharded mine; later unsharded mines filter it by their minsup
    // without a pass over the items (sharded mines neither fill nor read it)
    std::vector<uint32_t> f1_host;  // u32 [U]
    bool f1_made = false;
    // the DB-direct root (spade_engine.hip): offset in row << 16 | row length of every
    // entry, made by the first mine that needs it; pos_state 0 = not made, 1 = made,
    // -1 = a row exceeds 65535 entries (that DB keeps the root slab)
    fsm::DevBuf pos;      // u32 [E]
    int pos_state = 0;
    // the bounded root F2 plan's table (spade_engine.hip, k_f2_bound_tab): per row block b and
    // item u the sum of 1 + 3 (entries after it in its row) over u's entries in b, made by the
    // first mine that takes the bounded plan; f2_bound_rpb = the rows per block it was built
    // for (0 = not made; rebuilt when a mine's row block geometry differs); f2_bound_sum = the
    // sum of the whole table, read back once when it is built: with the regions' alignment it
    // bounds the key slots of every mine of this DB, whatever its minsup
    fsm::DevBuf f2_bound;  // u32 [row blocks * U]
    uint32_t f2_bound_rpb = 0;
    uint64_t f2_bound_sum = 0;
    // the vertical index (pattern_support.hip): item i's entries are vert[vert_off[i] ..
    // vert_off[i+1]), each (row, entry index); made by the first fsm_patterns_support on this
    // DB (vert_state 0 = not made, 1 = made, in no particular order inside a list, 2 = made
    // and every list in ascending row order: the first fsm_patterns_sids orders them).  The
    // host copy of vert_off gives the list lengths (= F1 supports) the pivot choice reads
    fsm::DevBuf vert_off;  // u32 [U+1]
    fsm::DevBuf vert;      // uint2 [E]
    std::vector<uint32_t> vert_off_host;
    int vert_state = 0;
    // the sequence id of every row (fsm_db::row_sid), uploaded by the first fsm_patterns_sids
    fsm::DevBuf row_sid;   // i32 [R]
    bool row_sid_made = false;
};

// TSR: horizontal rows (sid = row) of (item, first, last itemset index),
// item-sorted; the vertical transpose and sid bitmaps are built on the device.
struct TsrDevDB {
    fsm::DevBuf row_off, item, first, last;  // horizontal
    fsm::DevBuf vert_off, vert_sid, vert_item;
    fsm::DevBuf bm;                          // sid bitmaps: U x NW u32 (empty when over budget)
    int64_t N = 0, E = 0, U = 0;
    uint32_t NW = 0;                         // u32 words per item bitmap = ceil(N / 128) * 4 (16-byte rows)
    std::vector<uint32_t> sup;               // |sids(item)|
};

namespace fsm {
// tsr_engine.hip: vertical transpose + sid bitmaps + supports of a TSR DB whose rows are in HBM
void tsr_finish(fsm_ctx* ctx, TsrDevDB* d);
// k0_build.hip: K0 on the device from the token stream; false = this input takes the host flatten
bool k0_build(fsm_ctx* ctx, int mode, const Source& src, fsm_db* db);
}  // namespace fsm
