// rule_predict.hip — per row of a resident TSR DB, the items that GIVEN rules say should come
// next (fsm_rules_predict).
//
// By definition on the DB's rows (row = sequence = the caller's dense sid): rule r = X => Y
// fires in row s iff s holds every item of X, with fx = max over x in X of first_s(x); an item
// y of Y is open in s under r iff r fires and s does not hold y or last_s(y) <= fx.  The rules
// are ranked (confidence descending, support descending, index ascending: the host compares
// the doubles), the best rule of (s, y) is the lowest-ranked rule under which y is open in s,
// and the list of s is its items with a best rule, ordered by that rule's rank, then by item
// value, cut to topn.
//
// As in rule_support.hip only the rows of X's rarest item (the pivot) can fire a rule, so the
// work list of a rule is its pivot's sid list:
//
//   k_rp_match<false>  count pass, one wave per tile = one rule and kRpTile consecutive entries
//                      of its pivot's list, one candidate row per lane: a lane that holds X
//                      adds its number of open Y items to its row's counter.
//   k_scan             the rows' record segments and the total (read back: every buffer below
//                      is sized from it).
//   k_rp_match<true>   write pass, the same walk: a record (item ordinal << 32 | rank) goes to
//                      the row's segment through a per-row cursor.  The ordinal is the item's
//                      position among the call's ascending distinct Y values, so an item the
//                      DB does not hold orders by value like any other.
//   k_rp_sort          rocPRIM's segmented radix sort, twice: by (item, rank), then, after
//   k_rp_first         the first record of every item run (the item's best rule) is re-keyed
//                      (rank << 32 | ordinal) and every other record becomes one key above
//                      them all, by (rank, item).  The kept records lead their segment, so
//                      nothing is compacted.
//   k_rp_select        the first min(kept, topn) records of every row as (item value, rule
//                      index), and the final off.
//
// The order in which the atomics of the write pass land decides only where a record sits in
// its segment before the first sort; the records of a segment are distinct (a rule meets a
// row once, a rule's Y items are distinct), so the sorted segment, and with it the result, is
// the same every time.
//
// Record memory grows with the sum over rules of ante x |Y|, not with the output: a call whose
// records do not fit the scratch budget writes, sorts and selects one row range after the
// other (the count pass is shared; a lane of the write pass drops the rows outside its range).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <numeric>

#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "dev_db.h"
#include "device_util.h"
#include "host_pool.h"

namespace fsm {

namespace {

// --- geometry (the tests read these from this file) ---
constexpr int kRpTile = 64;             // candidate rows per tile = lanes of a wave
constexpr int kRpBlock = 256;           // threads per block: kRpBlock / kRpTile waves
constexpr unsigned kRpMaxGrid = 16384;  // blocks at most; the tiles / rows beyond are grid-strided
constexpr uint64_t kRpSliceTiles = 0xFFFFFFFFull;  // tiles per launch at most (u32 tile ids)
constexpr int kRpRecordBytes = 32;      // scratch per record: two key buffers and the sort's own
constexpr uint64_t kRpMaxRecords = 0x7FFFFFFFull;  // records per pass at most (the sort's u32 sizes)

constexpr uint32_t kRpDead = 0xFFFFFFFFu;  // pivot of a rule whose X cannot match (no tiles)

static_assert(kRpTile == 64, "a tile is one wave64");
static_assert(kRpBlock % kRpTile == 0, "whole waves");

// entry index of dense item `it` in the row's ascending items [b, e), kNone when absent
// (an unknown Y item is the token kNone: above every dense id, so it is never found)
__device__ __forceinline__ uint32_t rp_find(const uint32_t* __restrict__ item, uint32_t b, uint32_t e, uint32_t it) {
    uint32_t lo = b, hi = e;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (item[mid] < it) lo = mid + 1;
        else hi = mid;
    }
    return (lo < e && item[lo] == it) ? lo : kNone;
}

// Tiles as in k_rs_count: tile t (relative to this launch's first tile) belongs to the last
// rule r of [r0, r1) with toff[r] <= t.  Rule r has X = tok[ioff[2r] .. ioff[2r+1]) and
// Y = tok[ioff[2r+1] .. ioff[2r+2]), dense ids; yord[i] is the ordinal of Y token i.
// Only the rows of [row_a, row_b) are looked at.
//   kWrite false: cnt[row] += the row's open items under the tile's rule.
//   kWrite true:  cnt is the rows' cursors (zero before the call's first write launch); a
//                 record goes to keys[seg[row] + cursor - seg_base] if that lies inside the
//                 row's segment [seg[row], seg[row + 1]), else it is dropped and counted in
//                 tally[1]; tally[0] counts the records written.
template <bool kWrite>
__global__ __launch_bounds__(kRpBlock) void k_rp_match(
    const uint32_t* __restrict__ row_off, const uint32_t* __restrict__ item, const uint32_t* __restrict__ first,
    const uint32_t* __restrict__ last, const uint64_t* __restrict__ vert_off, const uint32_t* __restrict__ vert_sid,
    const uint32_t* __restrict__ tok, const uint32_t* __restrict__ yord, const uint32_t* __restrict__ ioff,
    const uint32_t* __restrict__ piv, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ toff, uint32_t r0,
    uint32_t r1, uint64_t ntiles, uint32_t row_a, uint32_t row_b, uint32_t* __restrict__ cnt,
    const uint64_t* __restrict__ seg, uint64_t seg_base, uint64_t* __restrict__ keys,
    unsigned long long* __restrict__ tally) {
    const uint64_t waves = uint64_t(gridDim.x) * (kRpBlock / kRpTile);
    for (uint64_t t64 = uint64_t(blockIdx.x) * (kRpBlock / kRpTile) + threadIdx.x / kRpTile; t64 < ntiles; t64 += waves) {
        const uint32_t t = uint32_t(t64);
        uint32_t lo = r0, hi = r1;
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (toff[mid] <= t) lo = mid;
            else hi = mid;
        }
        const uint32_t r = __builtin_amdgcn_readfirstlane(lo);
        const uint32_t xb = ioff[2 * uint64_t(r)], yb = ioff[2 * uint64_t(r) + 1], ye = ioff[2 * uint64_t(r) + 2];
        const uint32_t pv = piv[r];  // the pivot's dense id (a rule with tiles is not dead)
        const uint64_t lb = vert_off[pv];
        const uint32_t ln = uint32_t(vert_off[pv + 1] - lb);
        const uint32_t k = (t - toff[r]) * kRpTile + lane_id();
        bool alive = k < ln;
        uint32_t sid = 0, rb = 0, re = 0;
        if (alive) {
            sid = vert_sid[lb + k];
            alive = sid >= row_a && sid < row_b;
        }
        if (alive) {
            rb = row_off[sid];
            re = row_off[sid + 1];
        }
        uint32_t fx = 0;  // max of first over X
        for (uint32_t i = xb; i < yb && ballot(alive) != 0; ++i) {
            const uint32_t it = tok[i];
            if (alive) {
                const uint32_t en = rp_find(item, rb, re, it);
                alive = en != kNone;
                if (alive) fx = max(fx, first[en]);
            }
        }
        if (ballot(alive) == 0) continue;  // (wave-uniform: the rule fires in none of the tile's rows)
        uint32_t nopen = 0, dropped = 0;
        uint32_t rk = 0;
        uint64_t sb = 0, se = 0;
        if constexpr (kWrite) {
            rk = rank[r];
            if (alive) {
                sb = seg[sid];
                se = seg[uint64_t(sid) + 1];
            }
        }
        for (uint32_t i = yb; i < ye; ++i) {
            const uint32_t it = tok[i];
            if (alive) {
                const uint32_t en = rp_find(item, rb, re, it);
                if (en == kNone || last[en] <= fx) {  // y has not occurred strictly after X was complete
                    if constexpr (kWrite) {
                        const uint64_t p = sb + atomicAdd(&cnt[sid], 1u);
                        if (p < se) {
                            keys[p - seg_base] = (uint64_t(yord[i]) << 32) | rk;
                            ++nopen;
                        } else {
                            ++dropped;
                        }
                    } else {
                        ++nopen;
                    }
                }
            }
        }
        if constexpr (kWrite) {
            if (ballot(nopen != 0 || dropped != 0) != 0) {
                const uint32_t w = wave_incl_scan(nopen), dr = wave_incl_scan(dropped);
                if (lane_id() == 63) {
                    if (w) atomicAdd(&tally[0], (unsigned long long)w);
                    if (dr) atomicAdd(&tally[1], (unsigned long long)dr);
                }
            }
        } else {
            if (nopen) atomicAdd(&cnt[sid], nopen);
        }
    }
}

// One wave per row of [row_a, row_b): `sorted` holds the row's records in (ordinal, rank)
// order at [seg[row], seg[row + 1]) - seg_base.  The first record of every ordinal run is the
// item's best rule: it becomes rank << 32 | ordinal in `rekeyed`, every other record `dead`
// (above every kept key).  ocnt[row - row_a] = min(kept, topn).
__global__ __launch_bounds__(kRpBlock) void k_rp_first(const uint64_t* __restrict__ seg, uint64_t seg_base, uint32_t row_a,
                                                       uint32_t row_b, const uint64_t* __restrict__ sorted,
                                                       uint64_t* __restrict__ rekeyed, uint64_t dead, uint32_t topn,
                                                       uint32_t* __restrict__ ocnt) {
    const uint64_t waves = uint64_t(gridDim.x) * (kRpBlock / kRpTile);
    for (uint64_t row = row_a + uint64_t(blockIdx.x) * (kRpBlock / kRpTile) + threadIdx.x / kRpTile; row < row_b;
         row += waves) {
        const uint64_t s0 = seg[row] - seg_base, s1 = seg[row + 1] - seg_base;
        uint32_t kept = 0;
        for (uint64_t c = s0; c < s1; c += kRpTile) {  // (wave-uniform)
            const uint64_t i = c + lane_id();
            bool head = false;
            if (i < s1) {
                const uint64_t key = sorted[i];
                head = i == s0 || (sorted[i - 1] >> 32) != (key >> 32);
                rekeyed[i] = head ? ((key << 32) | (key >> 32)) : dead;
            }
            kept += uint32_t(__popcll(ballot(head)));
        }
        if (lane_id() == 0) ocnt[row - row_a] = min(kept, topn);
    }
}

// One wave per row of [row_a, row_b): `sorted` holds the row's kept records first, in (rank,
// ordinal) order; row's entries are its first ooff[row - row_a + 1] - ooff[row - row_a], written
// at ooff[row - row_a] as (item value, rule index).  off[row] = pbase + ooff[row - row_a], and
// the range's last row also writes off[row_b].
__global__ __launch_bounds__(kRpBlock) void k_rp_select(const uint64_t* __restrict__ seg, uint64_t seg_base, uint32_t row_a,
                                                        uint32_t row_b, const uint64_t* __restrict__ sorted,
                                                        const uint64_t* __restrict__ ooff, int64_t pbase,
                                                        const int32_t* __restrict__ yval,
                                                        const int32_t* __restrict__ rule_of_rank,
                                                        int32_t* __restrict__ out_item, int32_t* __restrict__ out_rule,
                                                        int64_t* __restrict__ off) {
    const uint64_t waves = uint64_t(gridDim.x) * (kRpBlock / kRpTile);
    for (uint64_t row = row_a + uint64_t(blockIdx.x) * (kRpBlock / kRpTile) + threadIdx.x / kRpTile; row < row_b;
         row += waves) {
        const uint64_t s0 = seg[row] - seg_base;
        const uint64_t o0 = ooff[row - row_a], o1 = ooff[row - row_a + 1];
        for (uint64_t j = lane_id(); j < o1 - o0; j += kRpTile) {
            const uint64_t key = sorted[s0 + j];
            out_item[o0 + j] = yval[uint32_t(key)];
            out_rule[o0 + j] = rule_of_rank[uint32_t(key >> 32)];
        }
        if (lane_id() == 0) {
            off[row] = pbase + int64_t(o0);
            if (row + 1 == row_b) off[row_b] = pbase + int64_t(o1);
        }
    }
}

unsigned rp_grid(uint64_t work, uint64_t per_block) {
    return unsigned(std::min<uint64_t>(std::max<uint64_t>((work + per_block - 1) / per_block, 1), kRpMaxGrid));
}

// a row's segment bound relative to its pass, as the sort's u32 offsets
struct RpRel {
    uint64_t base;
    __host__ __device__ unsigned int operator()(uint64_t v) const { return (unsigned int)(v - base); }
};

unsigned bits_for(uint64_t n) {  // bits that hold every value below n (n >= 1)
    unsigned b = 0;
    while (b < 64 && (uint64_t(1) << b) < n) ++b;
    return b;
}

// The environment of one call, read once (test hooks: they may change the speed, never a result):
//   FSM_RP_PIVOT=first|last   X's first / last item is the pivot whatever the list lengths
//   FSM_RP_SLICE_ROWS=<n>     n rows per pass (n >= 1; else ignored)
struct RpKnobs {
    int pivot = 0;  // 0 = the X item with the fewest sids, 1 = first, 2 = last
    uint64_t slice_rows = 0;  // 0 = as the scratch budget allows

    static RpKnobs from_env() {
        RpKnobs k;
        if (const char* v = std::getenv("FSM_RP_PIVOT")) k.pivot = !std::strcmp(v, "first") ? 1 : !std::strcmp(v, "last") ? 2 : 0;
        if (const char* v = std::getenv("FSM_RP_SLICE_ROWS")) {
            char* end = nullptr;
            const long long n = std::strtoll(v, &end, 10);
            if (end != v && !*end && n >= 1) k.slice_rows = uint64_t(n);
        }
        return k;
    }
};

}  // namespace

void rules_predict(fsm_ctx* ctx, fsm_db* db, const fsm_rules* in, int32_t topn, fsm_predictions** out) {
    const char* who = "fsm_rules_predict";
    const std::string w = std::string(who) + ": ";
    if (in->n >= (int64_t(1) << 31)) throw Error(FSM_ELIMIT, w + "2^31 or more rules");
    rules_validate(in, who);
    const int64_t n = in->n;
    if (n > 0) {
        if (!in->support || !in->confidence) throw Error(FSM_EINVAL, w + "null support or confidence");
        for (int64_t r = 0; r < n; ++r)
            if (std::isnan(in->confidence[r])) throw Error(FSM_EINVAL, w + "confidence of rule " + std::to_string(r) + " is not a number");
    }
    const RpKnobs kn = RpKnobs::from_env();
    TsrDevDB* d = db->tsr_dev;
    if (d->U >= (int64_t(1) << 31)) throw Error(FSM_ELIMIT, w + "2^31 or more distinct items in the DB");
    const size_t N = size_t(d->N);

    // the library-owned result; the arrays are released into it
    MallocArr<int64_t> r_off(N + 1);
    MallocArr<int32_t> r_item, r_rule;
    auto result = [&](int64_t total) {
        auto* r = static_cast<fsm_predictions*>(std::calloc(1, sizeof(fsm_predictions)));
        if (!r) throw Error(FSM_ENOMEM, "calloc failed");
        r->n = int64_t(N);
        r->n_preds = total;
        r->off = r_off.release();
        r->item = r_item.release();
        r->rule = r_rule.release();
        *out = r;
    };
    auto empty_result = [&] {
        std::memset(r_off.p, 0, (N + 1) * 8);
        r_item.alloc(0);
        r_rule.alloc(0);
        result(0);
    };
    if (n == 0 || N == 0) {
        ctx->kstats.clear();
        empty_result();
        return;
    }

    // the input is valid: ranks, Y ordinals, dense ids, pivots and tiles
    const std::vector<int32_t>& val = db->tsr.item_val;
    const std::vector<uint32_t>& len = d->sup;  // |sids(item)| = the length of its vertical list
    const size_t un = size_t(n), ui = size_t(in->ante_off[n] + in->cons_off[n]);
    // (the upload sources: declared ahead of the stream guard, which outlives no queued copy)
    std::vector<int32_t> ror(un);  // rule of rank
    std::iota(ror.begin(), ror.end(), 0);
    std::sort(ror.begin(), ror.end(), [&](int32_t a, int32_t b) {
        if (in->confidence[a] != in->confidence[b]) return in->confidence[a] > in->confidence[b];
        if (in->support[a] != in->support[b]) return in->support[a] > in->support[b];
        return a < b;
    });
    std::vector<uint32_t> rank(un);
    for (size_t k = 0; k < un; ++k) rank[size_t(ror[k])] = uint32_t(k);
    std::vector<int32_t> yval(in->cons, in->cons + in->cons_off[n]);  // the call's distinct Y values, ascending
    std::sort(yval.begin(), yval.end());
    yval.erase(std::unique(yval.begin(), yval.end()), yval.end());

    std::vector<uint32_t> tok(ui), yord(ui, 0), ioff(2 * un + 1), piv(un), toff;
    std::vector<uint64_t> tile_off(un + 1, 0);  // tiles of rule r at [r + 1], summed below
    auto dense = [&](int32_t v) {
        const auto it = std::lower_bound(val.begin(), val.end(), v);
        return (it == val.end() || *it != v) ? kNone : uint32_t(it - val.begin());
    };
    const int64_t nthr = n >= 65536 ? host_threads() : 1;
    par_slices(nthr, n, [&](int64_t, int64_t a, int64_t b) {
        for (int64_t r = a; r < b; ++r) {
            const int64_t x0 = in->ante_off[r], x1 = in->ante_off[r + 1], y0 = in->cons_off[r], y1 = in->cons_off[r + 1];
            const uint32_t i0 = uint32_t(x0 + y0);  // X then Y of a rule, rule after rule
            ioff[2 * size_t(r)] = i0;
            ioff[2 * size_t(r) + 1] = i0 + uint32_t(x1 - x0);
            bool live = true;
            uint32_t best = kRpDead, best_len = 0;
            for (int64_t i = x0; i < x1; ++i) {
                const uint32_t id = dense(in->ante[i]);
                tok[i0 + size_t(i - x0)] = id;
                if (id == kNone) {
                    live = false;  // (its tokens are never read: the rule gets no tile)
                    continue;
                }
                if (best == kRpDead || len[id] < best_len) {
                    best = id;
                    best_len = len[id];
                }
            }
            if (live && kn.pivot) {
                best = tok[kn.pivot == 1 ? i0 : i0 + size_t(x1 - x0) - 1];
                best_len = len[best];
            }
            // an unknown Y item stays kNone: no row holds it, so it is open wherever the rule fires
            for (int64_t i = y0; i < y1; ++i) {
                const size_t at = i0 + size_t(x1 - x0) + size_t(i - y0);
                tok[at] = dense(in->cons[i]);
                yord[at] = uint32_t(std::lower_bound(yval.begin(), yval.end(), in->cons[i]) - yval.begin());
            }
            piv[size_t(r)] = live ? best : kRpDead;
            tile_off[size_t(r) + 1] = live ? (uint64_t(best_len) + kRpTile - 1) / kRpTile : 0;
        }
    });
    ioff[2 * un] = uint32_t(ui);
    int64_t tests = 0, x_items = 0, y_items = 0;  // (rule, row) pairs and their rule items, for the bytes
    for (size_t r = 0; r < un; ++r) {
        if (piv[r] != kRpDead) {
            const int64_t l = len[piv[r]];
            tests += l;
            x_items += l * int64_t(ioff[2 * r + 1] - ioff[2 * r]);
            y_items += l * int64_t(ioff[2 * r + 2] - ioff[2 * r + 1]);
        }
        tile_off[r + 1] += tile_off[r];
    }
    const uint64_t total_tiles = tile_off[un];
    if (!total_tiles) {
        ctx->kstats.clear();
        empty_result();
        return;
    }

    std::vector<uint64_t> hseg;  // the rows' record offsets, read back when the call takes several passes
    struct Pass {
        uint32_t a, b;
        uint64_t base, recs;
        int64_t pbase = 0, preds = 0;
    };
    std::vector<Pass> passes;
    std::deque<MallocArr<int32_t>> h_item, h_rule;  // the passes' entries (one pass: the result itself)

    FSM_HIP(hipSetDevice(ctx->opts.device));
    hipStream_t s = ctx->stream;
    struct SyncOnExit {
        hipStream_t s;
        ~SyncOnExit() { (void)hipStreamSynchronize(s); }
    } sync_on_exit{s};
    KernelClock clock(s);
    ClockScope clock_scope(&clock);  // (the scans record into it)
    // launches of at most kRpSliceTiles tiles over whole rules (one rule has fewer than 2^26
    // tiles); toff is relative to its launch's first tile, so it fits 32 bits
    toff.resize(un);
    std::vector<std::pair<uint32_t, uint32_t>> slices;
    for (size_t a = 0; a < un;) {
        size_t b = a + 1;
        while (b < un && tile_off[b + 1] - tile_off[a] <= kRpSliceTiles) ++b;
        for (size_t r = a; r < b; ++r) toff[r] = uint32_t(tile_off[r] - tile_off[a]);
        slices.emplace_back(uint32_t(a), uint32_t(b));
        a = b;
    }
    const size_t ny = yval.size();
    DevBuf d_cnt(N * 4), d_cur(N * 4), d_seg((N + 1) * 8), d_ocnt(N * 4), d_ooff((N + 1) * 8), d_off((N + 1) * 8), d_tally(16);
    DevBuf d_tok(ui * 4), d_yord(ui * 4), d_ioff((2 * un + 1) * 4), d_piv(un * 4), d_rank(un * 4), d_toff(un * 4),
        d_yval(ny * 4), d_ror(un * 4);
    FSM_HIP(hipMemsetAsync(d_cnt.p, 0, N * 4, s));
    FSM_HIP(hipMemsetAsync(d_cur.p, 0, N * 4, s));
    FSM_HIP(hipMemsetAsync(d_tally.p, 0, 16, s));
    FSM_HIP(hipMemcpyAsync(d_tok.p, tok.data(), ui * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_yord.p, yord.data(), ui * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_ioff.p, ioff.data(), (2 * un + 1) * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_piv.p, piv.data(), un * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_rank.p, rank.data(), un * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_toff.p, toff.data(), un * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_yval.p, yval.data(), ny * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_ror.p, ror.data(), un * 4, hipMemcpyHostToDevice, s));

    auto match = [&](bool write, uint32_t row_a, uint32_t row_b, uint64_t seg_base, uint64_t* keys) {
        for (const auto& sl : slices) {
            const uint64_t nt = tile_off[sl.second] - tile_off[sl.first];
            if (!nt) continue;
            const dim3 grid(rp_grid(nt, kRpBlock / kRpTile)), block(kRpBlock);
            if (write)
                hipLaunchKernelGGL(k_rp_match<true>, grid, block, 0, s, d->row_off.as<uint32_t>(), d->item.as<uint32_t>(),
                                   d->first.as<uint32_t>(), d->last.as<uint32_t>(), d->vert_off.as<uint64_t>(),
                                   d->vert_sid.as<uint32_t>(), d_tok.as<uint32_t>(), d_yord.as<uint32_t>(),
                                   d_ioff.as<uint32_t>(), d_piv.as<uint32_t>(), d_rank.as<uint32_t>(),
                                   d_toff.as<uint32_t>(), sl.first, sl.second, nt, row_a, row_b, d_cur.as<uint32_t>(),
                                   d_seg.as<uint64_t>(), seg_base, keys, d_tally.as<unsigned long long>());
            else
                hipLaunchKernelGGL(k_rp_match<false>, grid, block, 0, s, d->row_off.as<uint32_t>(), d->item.as<uint32_t>(),
                                   d->first.as<uint32_t>(), d->last.as<uint32_t>(), d->vert_off.as<uint64_t>(),
                                   d->vert_sid.as<uint32_t>(), d_tok.as<uint32_t>(), d_yord.as<uint32_t>(),
                                   d_ioff.as<uint32_t>(), d_piv.as<uint32_t>(), d_rank.as<uint32_t>(),
                                   d_toff.as<uint32_t>(), sl.first, sl.second, nt, row_a, row_b, d_cnt.as<uint32_t>(),
                                   d_seg.as<uint64_t>(), seg_base, keys, d_tally.as<unsigned long long>());
            FSM_LAUNCHED("k_rp_match", s);
        }
    };
    // the walk's bytes, as if no lane retired early.  Per (rule, row) test: the sid (4) and the
    // row bounds (8); per rule item of a test: one item word (the search's last probe, 4) and its
    // first or last (4).  Per tile: its rule's three offsets, pivot, rank and tile offset (24)
    // and the list bounds (16)
    const int64_t walk_bytes = tests * 12 + (x_items + y_items) * 8 + int64_t(total_tiles) * 40;

    // the count pass over every row, the rows' segments and the total
    uint64_t* pin = ctx->pinned_u64();
    {
        const size_t tk = clock.begin("k_rp_match");
        match(false, 0, uint32_t(N), 0, nullptr);
        clock.end(tk, walk_bytes + tests * 4);  // and one counter add per test
    }
    scan_exclusive(d_cnt.as<uint32_t>(), d_seg.as<uint64_t>(), N, s);
    FSM_HIP(hipMemcpyAsync(pin, d_seg.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost, s));
    FSM_HIP(hipStreamSynchronize(s));
    const uint64_t total = pin[0];
    if (!total) {
        clock.finish(ctx->kstats);
        empty_result();
        return;
    }

    // the passes: row ranges whose records fit the scratch budget (a row with more is a pass of
    // its own), or of slice_rows rows; ranges without a record need no pass
    size_t free_b = 0, total_b = 0;
    FSM_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = ctx->opts.mem_budget > 0 ? uint64_t(ctx->opts.mem_budget) : uint64_t(free_b / 2) / uint64_t(ctx->dev_share);
    const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(budget / kRpRecordBytes, 1), kRpMaxRecords);
    if (!kn.slice_rows && total <= cap) {
        passes.push_back(Pass{0, uint32_t(N), 0, total});
    } else {
        hseg.resize(N + 1);
        FSM_HIP(hipMemcpyAsync(hseg.data(), d_seg.p, (N + 1) * 8, hipMemcpyDeviceToHost, s));
        FSM_HIP(hipStreamSynchronize(s));
        const uint64_t max_rows = kn.slice_rows ? kn.slice_rows : uint64_t(N);
        for (size_t a = 0; a < N;) {
            size_t b = a + 1;
            while (b < N && b - a < max_rows && hseg[b + 1] - hseg[a] <= cap) ++b;
            if (hseg[b] - hseg[a] > kRpMaxRecords)
                throw Error(FSM_ELIMIT, w + "2^31 or more (rule, open item) records in one row");
            passes.push_back(Pass{uint32_t(a), uint32_t(b), hseg[a], hseg[b] - hseg[a]});
            a = b;
        }
    }

    const unsigned ord_bits = bits_for(ny), rank_bits = bits_for(un);
    const uint64_t dead = uint64_t(1) << (32 + rank_bits);  // above every rank << 32 | ordinal
    int64_t pbase = 0;
    uint64_t written = 0;
    for (Pass& ps : passes) {
        ps.pbase = pbase;
        if (!ps.recs) continue;
        const uint32_t nrows = ps.b - ps.a;
        const uint64_t R = ps.recs;
        DevBuf ka(R * 8), kb(R * 8);
        {
            const size_t tk = clock.begin("k_rp_match");
            match(true, ps.a, ps.b, ps.base, ka.as<uint64_t>());
            // and per record: its row's two segment bounds and cursor add (20), the ordinal (4), the key (8)
            clock.end(tk, walk_bytes + int64_t(R) * 32);
        }
        const auto seg_lo = rocprim::make_transform_iterator(d_seg.as<uint64_t>() + ps.a, RpRel{ps.base});
        const auto seg_hi = rocprim::make_transform_iterator(d_seg.as<uint64_t>() + ps.a + 1, RpRel{ps.base});
        size_t t1 = 0, t2 = 0;
        FSM_HIP(rocprim::segmented_radix_sort_keys(nullptr, t1, ka.as<uint64_t>(), kb.as<uint64_t>(), unsigned(R), nrows,
                                                   seg_lo, seg_hi, 0u, 32u + ord_bits, s));
        FSM_HIP(rocprim::segmented_radix_sort_keys(nullptr, t2, ka.as<uint64_t>(), kb.as<uint64_t>(), unsigned(R), nrows,
                                                   seg_lo, seg_hi, 0u, 33u + rank_bits, s));
        DevBuf tmp(std::max<size_t>(std::max(t1, t2), 16));
        const dim3 rgrid(rp_grid(nrows, kRpBlock / kRpTile)), block(kRpBlock);
        {  // by (item, rank): the first record of an item run is the item's best rule
            const size_t tk = clock.begin("k_rp_sort");
            FSM_HIP(rocprim::segmented_radix_sort_keys(tmp.p, t1, ka.as<uint64_t>(), kb.as<uint64_t>(), unsigned(R), nrows,
                                                       seg_lo, seg_hi, 0u, 32u + ord_bits, s));
            clock.end(tk, int64_t(R) * 16 + int64_t(nrows) * 16);  // keys in and out, the segment bounds
        }
        {
            const size_t tk = clock.begin("k_rp_first");
            hipLaunchKernelGGL(k_rp_first, rgrid, block, 0, s, d_seg.as<uint64_t>(), ps.base, ps.a, ps.b, kb.as<uint64_t>(),
                               ka.as<uint64_t>(), dead, uint32_t(topn), d_ocnt.as<uint32_t>());
            FSM_LAUNCHED("k_rp_first", s);
            // per record: its key, its neighbour's (from cache) and the new key; per row: two bounds, one count
            clock.end(tk, int64_t(R) * 16 + int64_t(nrows) * 20);
        }
        scan_exclusive(d_ocnt.as<uint32_t>(), d_ooff.as<uint64_t>(), nrows, s);
        {  // by (rank, item): the kept records lead their segment
            const size_t tk = clock.begin("k_rp_sort");
            FSM_HIP(rocprim::segmented_radix_sort_keys(tmp.p, t2, ka.as<uint64_t>(), kb.as<uint64_t>(), unsigned(R), nrows,
                                                       seg_lo, seg_hi, 0u, 33u + rank_bits, s));
            clock.end(tk, int64_t(R) * 16 + int64_t(nrows) * 16);
        }
        FSM_HIP(hipMemcpyAsync(pin, d_ooff.as<uint64_t>() + nrows, 8, hipMemcpyDeviceToHost, s));
        FSM_HIP(hipMemcpyAsync(pin + 1, d_tally.p, 16, hipMemcpyDeviceToHost, s));
        FSM_HIP(hipStreamSynchronize(s));
        // every record of the pass was written inside its row's segment, none was dropped: else
        // the segments hold something else than the count pass saw, and nothing is selected
        written += R;
        if (pin[1] != written || pin[2] != 0)
            throw Error(FSM_EDEVICE, w + "the write pass wrote " + std::to_string(pin[1]) + " records and dropped " +
                                         std::to_string(pin[2]) + ", the count pass had " + std::to_string(written));
        const uint64_t P = pin[0];
        ps.preds = int64_t(P);
        h_item.emplace_back(size_t(P));
        h_rule.emplace_back(size_t(P));
        DevBuf o_item(std::max<size_t>(size_t(P), 1) * 4), o_rule(std::max<size_t>(size_t(P), 1) * 4);
        {
            const size_t tk = clock.begin("k_rp_select");
            hipLaunchKernelGGL(k_rp_select, rgrid, block, 0, s, d_seg.as<uint64_t>(), ps.base, ps.a, ps.b, kb.as<uint64_t>(),
                               d_ooff.as<uint64_t>(), pbase, d_yval.as<int32_t>(), d_ror.as<int32_t>(), o_item.as<int32_t>(),
                               o_rule.as<int32_t>(), d_off.as<int64_t>());
            FSM_LAUNCHED("k_rp_select", s);
            // per row: its segment bound, two entry offsets and its off (32); per entry: the key, the item
            // value, the rule index and the two stores (24)
            clock.end(tk, int64_t(nrows) * 32 + int64_t(P) * 24);
        }
        if (P) {
            FSM_HIP(hipMemcpyAsync(h_item.back().p, o_item.p, size_t(P) * 4, hipMemcpyDeviceToHost, s));
            FSM_HIP(hipMemcpyAsync(h_rule.back().p, o_rule.p, size_t(P) * 4, hipMemcpyDeviceToHost, s));
        }
        FSM_HIP(hipStreamSynchronize(s));  // (the pass's buffers go back to the pool behind it)
        pbase += int64_t(P);
    }
    FSM_HIP(hipMemcpyAsync(r_off.p, d_off.p, (N + 1) * 8, hipMemcpyDeviceToHost, s));
    clock.finish(ctx->kstats);  // synchronizes the stream
    // the ranges without a pass: every off of theirs is the entries ahead of them
    for (const Pass& ps : passes)
        if (!ps.recs)
            for (size_t row = ps.a; row <= ps.b; ++row) r_off[row] = ps.pbase;
    if (h_item.size() == 1) {
        r_item.p = h_item[0].release();
        r_rule.p = h_rule[0].release();
    } else {
        r_item.alloc(size_t(pbase));
        r_rule.alloc(size_t(pbase));
        size_t k = 0;
        for (const Pass& ps : passes) {
            if (!ps.recs) continue;
            if (ps.preds) {
                std::memcpy(r_item.p + ps.pbase, h_item[k].p, size_t(ps.preds) * 4);
                std::memcpy(r_rule.p + ps.pbase, h_rule[k].p, size_t(ps.preds) * 4);
            }
            ++k;
        }
    }
    result(pbase);
}

}  // namespace fsm
