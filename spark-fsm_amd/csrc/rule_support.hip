// rule_support.hip — support, antecedent count and confidence of GIVEN rules in a resident
// TSR DB (fsm_rules_support).
//
// Counted by definition on the DB's rows (row = sequence): for r = X => Y,
//   ante(r)    = #rows holding every item of X
//   support(r) = #rows holding every item of X and of Y with
//                max over x in X of first_x  <  min over y in Y of last_y   (strict)
// The DB keeps, per row, its distinct items (ascending dense id) with the index of the first
// and of the last itemset they occur in, and per item the list of its sids (vert_off /
// vert_sid, made with the DB), so no index is built here.
//
// Only rows that hold X's rarest item (the rule's pivot) can hold X, and ante counts exactly
// the rows that hold X, so the work list of a rule is the pivot's sid list:
//
//   k_rs_count   one wave per tile = one rule and kRsTile consecutive entries of its pivot's
//                list, one candidate row per lane.  A lane searches every X item in its row
//                (max of first), then every Y item (min of last); the ballot popcount of the
//                lanes that hold X goes to the rule's ante counter, that of the lanes that
//                also pass first_X < last_Y to its support counter: two integer atomics per
//                tile at most.
//
// first / last are read as the u32 they are stored as (the miner's bitmap path packs them to
// 16 bits; nothing is packed here), and a side is read from memory item by item, so its
// length has no limit (the miner's kMaxSide is the size of its fixed Side arrays).
// The order inside a sid list depends on the transpose's atomics; a count does not (every
// list entry is tested on its own and integer adds commute).
#include <cstdio>
#include <cstring>

#include "dev_db.h"
#include "device_util.h"
#include "host_pool.h"

namespace fsm {

namespace {

// --- geometry (the tests read these from this file) ---
constexpr int kRsTile = 64;            // candidate rows per tile = lanes of a wave
constexpr int kRsBlock = 256;          // threads per block: kRsBlock / kRsTile tiles per block pass
constexpr unsigned kRsMaxGrid = 16384;  // blocks at most; the tiles beyond are grid-strided
constexpr uint64_t kRsSliceTiles = 0xFFFFFFFFull;  // tiles per launch at most (u32 tile ids)

constexpr uint32_t kRsDead = 0xFFFFFFFFu;  // pivot of a rule whose X cannot match (no tiles)

static_assert(kRsTile == 64, "a tile is one wave64");
static_assert(kRsBlock % kRsTile == 0, "whole waves");

// entry index of dense item `it` in the row's ascending items [b, e), kNone when absent
// (an unknown Y item is the token kNone: above every dense id, so it is never found)
__device__ __forceinline__ uint32_t rs_find(const uint32_t* __restrict__ item, uint32_t b, uint32_t e, uint32_t it) {
    uint32_t lo = b, hi = e;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (item[mid] < it) lo = mid + 1;
        else hi = mid;
    }
    return (lo < e && item[lo] == it) ? lo : kNone;
}

// Tile t (relative to this launch's first tile) belongs to the last rule r of [r0, r1) with
// toff[r] <= t; toff[r0] = 0 and rules without tiles repeat their successor's value.
// Rule r has X = tok[ioff[2r] .. ioff[2r+1]) and Y = tok[ioff[2r+1] .. ioff[2r+2]), dense ids;
// cnt[2r] counts its ante, cnt[2r+1] its support.
__global__ __launch_bounds__(kRsBlock) void k_rs_count(const uint32_t* __restrict__ row_off,
                                                       const uint32_t* __restrict__ item,
                                                       const uint32_t* __restrict__ first,
                                                       const uint32_t* __restrict__ last,
                                                       const uint64_t* __restrict__ vert_off,
                                                       const uint32_t* __restrict__ vert_sid,
                                                       const uint32_t* __restrict__ tok,
                                                       const uint32_t* __restrict__ ioff,
                                                       const uint32_t* __restrict__ piv,
                                                       const uint32_t* __restrict__ toff, uint32_t r0, uint32_t r1,
                                                       uint64_t ntiles, uint32_t* __restrict__ cnt) {
    const uint64_t waves = uint64_t(gridDim.x) * (kRsBlock / kRsTile);
    for (uint64_t t64 = uint64_t(blockIdx.x) * (kRsBlock / kRsTile) + threadIdx.x / kRsTile; t64 < ntiles; t64 += waves) {
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
        const uint32_t k = (t - toff[r]) * kRsTile + lane_id();
        bool alive = k < ln;
        uint32_t rb = 0, re = 0;
        if (alive) {
            const uint32_t sid = vert_sid[lb + k];
            rb = row_off[sid];
            re = row_off[sid + 1];
        }
        // the tokens are wave-uniform and read as the walk goes
        uint32_t fx = 0;  // max of first over X
        for (uint32_t i = xb; i < yb && ballot(alive) != 0; ++i) {
            const uint32_t it = tok[i];
            if (alive) {
                const uint32_t en = rs_find(item, rb, re, it);
                alive = en != kNone;
                if (alive) fx = max(fx, first[en]);
            }
        }
        const uint64_t holds_x = ballot(alive);
        if (holds_x == 0) continue;  // (wave-uniform)
        if (lane_id() == 0) atomicAdd(&cnt[2 * uint64_t(r)], uint32_t(__popcll(holds_x)));
        uint32_t ly = 0xFFFFFFFFu;  // min of last over Y (Y is not empty)
        for (uint32_t i = yb; i < ye && ballot(alive) != 0; ++i) {
            const uint32_t it = tok[i];
            if (alive) {
                const uint32_t en = rs_find(item, rb, re, it);
                alive = en != kNone;
                if (alive) ly = min(ly, last[en]);
            }
        }
        const uint64_t holds = ballot(alive && fx < ly);
        if (holds != 0 && lane_id() == 0) atomicAdd(&cnt[2 * uint64_t(r) + 1], uint32_t(__popcll(holds)));
    }
}

unsigned rs_grid(uint64_t work, uint64_t per_block) {
    return unsigned(std::min<uint64_t>(std::max<uint64_t>((work + per_block - 1) / per_block, 1), kRsMaxGrid));
}

// The environment of one call, read once (test hooks: they may change the speed, never a count):
//   FSM_RS_PIVOT=first|last   X's first / last item is the pivot whatever the list lengths
//   FSM_RS_SLICE_TILES=<n>    tiles per launch at most, [1, kRsSliceTiles] (else ignored)
struct RsKnobs {
    int pivot = 0;  // 0 = the X item with the fewest sids, 1 = first, 2 = last
    uint64_t slice_tiles = kRsSliceTiles;

    static RsKnobs from_env() {
        RsKnobs k;
        if (const char* v = std::getenv("FSM_RS_PIVOT")) k.pivot = !std::strcmp(v, "first") ? 1 : !std::strcmp(v, "last") ? 2 : 0;
        if (const char* v = std::getenv("FSM_RS_SLICE_TILES")) {
            char* end = nullptr;
            const long long n = std::strtoll(v, &end, 10);
            if (end != v && !*end && n >= 1 && uint64_t(n) <= kRsSliceTiles) k.slice_tiles = uint64_t(n);
        }
        return k;
    }
};

// The CSR checks (FSM_EINVAL / FSM_ELIMIT with `who` in front of the message), offsets before
// items: a size over the limit is refused before any item is read.
void rs_validate(const fsm_rules* in, const char* who) {
    const std::string w = std::string(who) + ": ";
    const int64_t n = in->n;
    if (n < 0) throw Error(FSM_EINVAL, w + "negative sizes");
    constexpr int64_t kLimit = (int64_t(1) << 32) - 2;
    if (n >= kLimit) throw Error(FSM_ELIMIT, w + "2^32 - 2 or more rules");
    if (n == 0) return;
    if (!in->ante_off || !in->cons_off || !in->ante || !in->cons) throw Error(FSM_EINVAL, w + "null rule arrays");
    if (in->ante_off[0] != 0 || in->cons_off[0] != 0) throw Error(FSM_EINVAL, w + "offsets must start at 0");
    for (int64_t r = 0; r < n; ++r) {
        if (in->ante_off[r + 1] < in->ante_off[r]) throw Error(FSM_EINVAL, w + "ante_off is not monotone at rule " + std::to_string(r));
        if (in->cons_off[r + 1] < in->cons_off[r]) throw Error(FSM_EINVAL, w + "cons_off is not monotone at rule " + std::to_string(r));
    }
    if (in->ante_off[n] >= kLimit || in->cons_off[n] >= kLimit || in->ante_off[n] + in->cons_off[n] >= kLimit)
        throw Error(FSM_ELIMIT, w + "2^32 - 2 or more items");
    const int64_t nthr = n >= 65536 ? host_threads() : 1;
    std::vector<int64_t> bad(size_t(nthr), -1);  // first bad rule of each slice
    std::vector<int> why(size_t(nthr), 0);
    par_slices(nthr, n, [&](int64_t th, int64_t a, int64_t b) {
        for (int64_t r = a; r < b && bad[size_t(th)] < 0; ++r) {
            const int64_t x0 = in->ante_off[r], x1 = in->ante_off[r + 1], y0 = in->cons_off[r], y1 = in->cons_off[r + 1];
            int e = 0;
            if (x0 == x1) e = 1;
            else if (y0 == y1) e = 2;
            for (int64_t i = x0 + 1; i < x1 && !e; ++i)
                if (in->ante[i] <= in->ante[i - 1]) e = 3;
            for (int64_t i = y0 + 1; i < y1 && !e; ++i)
                if (in->cons[i] <= in->cons[i - 1]) e = 4;
            for (int64_t i = x0, j = y0; i < x1 && j < y1 && !e;) {  // both ascending: a merge finds a shared item
                if (in->ante[i] == in->cons[j]) e = 5;
                else if (in->ante[i] < in->cons[j]) ++i;
                else ++j;
            }
            if (e) {
                bad[size_t(th)] = r;
                why[size_t(th)] = e;
            }
        }
    });
    static const char* const kWhy[] = {"", "an empty antecedent", "an empty consequent",
                                       "antecedent items not strictly ascending", "consequent items not strictly ascending",
                                       "an item on both sides"};
    for (size_t th = 0; th < bad.size(); ++th)
        if (bad[th] >= 0) throw Error(FSM_EINVAL, w + kWhy[why[th]] + " in rule " + std::to_string(bad[th]));
}

}  // namespace

void rules_validate(const fsm_rules* in, const char* who) { rs_validate(in, who); }

void rules_support(fsm_ctx* ctx, fsm_db* db, const fsm_rules* in, int32_t* support_out, int32_t* ante_out,
                   double* confidence_out) {
    const char* who = "fsm_rules_support";
    rs_validate(in, who);
    const int64_t n = in->n;
    if (n == 0) {
        ctx->kstats.clear();
        return;
    }
    const RsKnobs kn = RsKnobs::from_env();

    // the input is valid: dense ids, pivots and tiles, split over the host threads by rules
    TsrDevDB* d = db->tsr_dev;
    if (d->U >= (int64_t(1) << 31)) throw Error(FSM_ELIMIT, std::string(who) + ": 2^31 or more distinct items in the DB");
    const std::vector<int32_t>& val = db->tsr.item_val;
    const std::vector<uint32_t>& len = d->sup;  // |sids(item)| = the length of its vertical list
    const size_t un = size_t(n), ui = size_t(in->ante_off[n] + in->cons_off[n]);
    // (the upload sources: declared ahead of the stream guard, which outlives no queued copy)
    std::vector<uint32_t> tok(ui), ioff(2 * un + 1), piv(un), toff;
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
            uint32_t best = kRsDead, best_len = 0;
            for (int64_t i = x0; i < x1; ++i) {
                const uint32_t id = dense(in->ante[i]);
                tok[i0 + size_t(i - x0)] = id;
                if (id == kNone) {
                    live = false;  // (its tokens are never read: the rule gets no tile)
                    continue;
                }
                if (best == kRsDead || len[id] < best_len) {
                    best = id;
                    best_len = len[id];
                }
            }
            if (live && kn.pivot) {
                best = tok[kn.pivot == 1 ? i0 : i0 + size_t(x1 - x0) - 1];
                best_len = len[best];
            }
            // an unknown Y item stays kNone: no row holds it, and ante still counts
            for (int64_t i = y0; i < y1; ++i) tok[i0 + size_t(x1 - x0) + size_t(i - y0)] = dense(in->cons[i]);
            piv[size_t(r)] = live ? best : kRsDead;
            tile_off[size_t(r) + 1] = live ? (uint64_t(best_len) + kRsTile - 1) / kRsTile : 0;
        }
    });
    ioff[2 * un] = uint32_t(ui);
    int64_t tests = 0, live_items = 0;  // (rule, row) pairs and their rule items, for the bytes
    for (size_t r = 0; r < un; ++r) {
        if (piv[r] != kRsDead) {
            const int64_t l = len[piv[r]];
            tests += l;
            live_items += l * int64_t(ioff[2 * r + 2] - ioff[2 * r]);
        }
        tile_off[r + 1] += tile_off[r];
    }
    const uint64_t total_tiles = tile_off[un];

    std::vector<uint32_t> cnt(2 * un, 0);
    if (total_tiles) {
        FSM_HIP(hipSetDevice(ctx->opts.device));
        hipStream_t s = ctx->stream;
        struct SyncOnExit {
            hipStream_t s;
            ~SyncOnExit() { (void)hipStreamSynchronize(s); }
        } sync_on_exit{s};
        KernelClock clock(s);
        // launches of at most slice_tiles tiles over whole rules (one rule has fewer than 2^26
        // tiles); toff is relative to its launch's first tile, so it fits 32 bits
        toff.resize(un);
        std::vector<std::pair<uint32_t, uint32_t>> slices;
        for (size_t a = 0; a < un;) {
            size_t b = a + 1;
            while (b < un && tile_off[b + 1] - tile_off[a] <= kn.slice_tiles) ++b;
            for (size_t r = a; r < b; ++r) toff[r] = uint32_t(tile_off[r] - tile_off[a]);
            slices.emplace_back(uint32_t(a), uint32_t(b));
            a = b;
        }
        DevBuf d_cnt(2 * un * 4), d_tok(ui * 4), d_ioff((2 * un + 1) * 4), d_piv(un * 4), d_toff(un * 4);
        FSM_HIP(hipMemsetAsync(d_cnt.p, 0, 2 * un * 4, s));
        FSM_HIP(hipMemcpyAsync(d_tok.p, tok.data(), ui * 4, hipMemcpyHostToDevice, s));
        FSM_HIP(hipMemcpyAsync(d_ioff.p, ioff.data(), (2 * un + 1) * 4, hipMemcpyHostToDevice, s));
        FSM_HIP(hipMemcpyAsync(d_piv.p, piv.data(), un * 4, hipMemcpyHostToDevice, s));
        FSM_HIP(hipMemcpyAsync(d_toff.p, toff.data(), un * 4, hipMemcpyHostToDevice, s));
        const size_t tk = clock.begin("k_rs_count");
        for (const auto& sl : slices) {
            const uint64_t nt = tile_off[sl.second] - tile_off[sl.first];
            if (!nt) continue;
            hipLaunchKernelGGL(k_rs_count, dim3(rs_grid(nt, kRsBlock / kRsTile)), dim3(kRsBlock), 0, s,
                               d->row_off.as<uint32_t>(), d->item.as<uint32_t>(), d->first.as<uint32_t>(),
                               d->last.as<uint32_t>(), d->vert_off.as<uint64_t>(), d->vert_sid.as<uint32_t>(),
                               d_tok.as<uint32_t>(), d_ioff.as<uint32_t>(), d_piv.as<uint32_t>(), d_toff.as<uint32_t>(),
                               sl.first, sl.second, nt, d_cnt.as<uint32_t>());
            FSM_LAUNCHED("k_rs_count", s);
        }
        // as if no lane retired early.  Per (rule, row) test: the sid (4) and the row bounds (8);
        // per rule item of a test: one item word (the search's last probe, 4) and its first or
        // last (4).  Per tile: its rule's three offsets, pivot and tile offset (20), the list
        // bounds (16) and two counter adds (8)
        clock.end(tk, tests * 12 + live_items * 8 + int64_t(total_tiles) * 44);
        FSM_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, 2 * un * 4, hipMemcpyDeviceToHost, s));
        clock.finish(ctx->kstats);  // synchronizes the stream
    } else {
        ctx->kstats.clear();
    }
    for (size_t r = 0; r < un; ++r) {
        const uint32_t nx = cnt[2 * r], sup = cnt[2 * r + 1];
        support_out[r] = int32_t(sup);
        if (ante_out) ante_out[r] = int32_t(nx);
        // the miner's own expression (tsr_engine.hip): a mined rule scores bit-equal
        if (confidence_out) confidence_out[r] = nx ? double(sup) / double(nx) : 0.0;
    }
}

}  // namespace fsm
