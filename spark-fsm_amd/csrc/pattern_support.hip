// pattern_support.hip — supports of GIVEN patterns in a resident SPADE DB
// (fsm_patterns_support).
//
// Support is counted by definition: P = <X1 ... Xm> is contained in a row iff
// eids e1 < ... < em exist with every item of Xk present at ek.  The DB keeps, per row, its
// distinct items (ascending dense id) with the mask of the eids they occur at, so the
// containment test of one (pattern, row) pair is a greedy walk: AND the masks of Xk's items,
// take the lowest set eid strictly above e(k-1).  Taking the earliest eid every time is
// exact: whatever embedding exists, the greedy one ends no later at every k.
//
// Only rows that hold the pattern's rarest item (its pivot) can contain it, so the work
// list of a pattern is the pivot's list in a vertical index (item -> its (row, entry)
// pairs), which the first call on a DB builds on the device and the DB keeps:
//
//   k_ps_index_hist     entries per item (one integer atomic per DB entry)
//   k_scan              fsm::scan_exclusive over the histogram
//   k_ps_index_off      the u64 offsets narrowed to vert_off (E < 2^32) and a cursor copy
//   k_ps_index_scatter  one wave per row: (row, entry) to the item's next free slot
//
//   k_ps_count          one wave per tile = one pattern and kPsTile consecutive entries of
//                       its pivot's list, one candidate row per lane; the survivors' ballot
//                       popcount goes to the pattern's counter with one integer atomic
//
// The order inside a vertical list depends on the scatter's atomics; a count does not
// (every list entry is tested on its own and integer adds commute).
#include <cstdio>
#include <cstring>

#include "dev_db.h"
#include "device_util.h"
#include "host_pool.h"

namespace fsm {

namespace {

// --- geometry (the tests read these from this file) ---
constexpr int kPsTile = 64;           // candidate rows per tile = lanes of a wave
constexpr int kPsBlock = 256;         // threads per block: kPsBlock / kPsTile tiles per block pass
constexpr unsigned kPsMaxGrid = 16384;  // blocks at most; the tiles beyond are grid-strided
constexpr int kPsSetRegs = 8;         // W > 1: entry indexes of an itemset kept in registers
constexpr uint64_t kPsSliceTiles = 0xFFFFFFFFull;  // tiles per launch at most (u32 tile ids)

constexpr uint32_t kPsOpen = 0x80000000u;  // token: dense item id | kPsOpen when it opens an itemset
constexpr uint32_t kPsDead = 0xFFFFFFFFu;  // pivot of a pattern that cannot match

static_assert(kPsTile == 64, "a tile is one wave64");
static_assert(kPsBlock % kPsTile == 0, "whole waves");

// ---------------------------------------------------------------- vertical index
__global__ __launch_bounds__(kPsBlock) void k_ps_index_hist(const uint32_t* __restrict__ item, uint32_t E,
                                                            uint32_t* __restrict__ cnt) {
    const uint64_t stride = uint64_t(gridDim.x) * kPsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kPsBlock + threadIdx.x; i < E; i += stride) atomicAdd(&cnt[item[i]], 1u);
}

__global__ __launch_bounds__(kPsBlock) void k_ps_index_off(const uint64_t* __restrict__ off, uint32_t n,
                                                           uint32_t* __restrict__ vert_off,
                                                           uint32_t* __restrict__ cursor) {
    const uint64_t stride = uint64_t(gridDim.x) * kPsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kPsBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t v = uint32_t(off[i]);
        vert_off[i] = v;
        cursor[i] = v;  // (cursor has n entries too; its last one is never advanced)
    }
}

__global__ __launch_bounds__(kPsBlock) void k_ps_index_scatter(const uint32_t* __restrict__ row_off,
                                                               const uint32_t* __restrict__ item, uint32_t R,
                                                               uint32_t* __restrict__ cursor,
                                                               uint2* __restrict__ vert) {
    const uint64_t waves = uint64_t(gridDim.x) * (kPsBlock / 64);
    for (uint64_t r = uint64_t(blockIdx.x) * (kPsBlock / 64) + threadIdx.x / 64; r < R; r += waves) {
        const uint32_t b = row_off[r], e = row_off[r + 1];
        for (uint32_t i = b + lane_id(); i < e; i += 64) {
            const uint32_t slot = atomicAdd(&cursor[item[i]], 1u);
            vert[slot] = make_uint2(uint32_t(r), i);
        }
    }
}

// ---------------------------------------------------------------- count
// entry index of dense item `it` in the row's ascending items [b, e), kNone when absent
__device__ __forceinline__ uint32_t ps_find(const uint32_t* __restrict__ item, uint32_t b, uint32_t e, uint32_t it) {
    uint32_t lo = b, hi = e;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (item[mid] < it) lo = mid + 1;
        else hi = mid;
    }
    return (lo < e && item[lo] == it) ? lo : kNone;
}

// Tile t (relative to this launch's first tile) belongs to the last pattern p of [p0, p1)
// with toff[p] <= t; toff[p0] = 0 and patterns without tiles repeat their successor's value.
// W1: one-word masks (the AND stays in a register); otherwise `wd` words per mask, walked
// from the previous eid's word on.
template <bool W1>
__global__ __launch_bounds__(kPsBlock) void k_ps_count(const uint32_t* __restrict__ row_off,
                                                       const uint32_t* __restrict__ item,
                                                       const uint64_t* __restrict__ mask, uint32_t wd,
                                                       const uint32_t* __restrict__ vert_off,
                                                       const uint2* __restrict__ vert,
                                                       const uint32_t* __restrict__ tok,
                                                       const uint32_t* __restrict__ ioff,
                                                       const uint32_t* __restrict__ piv,
                                                       const uint32_t* __restrict__ toff, uint32_t p0, uint32_t p1,
                                                       uint64_t ntiles, int32_t* __restrict__ count) {
    const uint64_t waves = uint64_t(gridDim.x) * (kPsBlock / kPsTile);
    for (uint64_t t64 = uint64_t(blockIdx.x) * (kPsBlock / kPsTile) + threadIdx.x / kPsTile; t64 < ntiles; t64 += waves) {
        const uint32_t t = uint32_t(t64);
        uint32_t lo = p0, hi = p1;
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (toff[mid] <= t) lo = mid;
            else hi = mid;
        }
        const uint32_t p = __builtin_amdgcn_readfirstlane(lo);
        const uint32_t ib = ioff[p], ie = ioff[p + 1];
        const uint32_t pv = tok[piv[p]] & ~kPsOpen;  // the pivot's dense id
        const uint32_t lb = vert_off[pv], ln = vert_off[pv + 1] - lb;
        const uint32_t k = (t - toff[p]) * kPsTile + lane_id();
        bool alive = k < ln;
        uint32_t rb = 0, re = 0, pent = 0;
        if (alive) {
            const uint2 v = vert[lb + k];
            rb = row_off[v.x];
            re = row_off[v.x + 1];
            pent = v.y;
        }
        int32_t prev = -1;  // eid taken for the previous itemset
        // itemset by itemset; the tokens are wave-uniform and read as the walk goes
        for (uint32_t i = ib; i < ie && ballot(alive) != 0;) {
            uint32_t j = i + 1;
            while (j < ie && !(tok[j] & kPsOpen)) ++j;  // [i, j) is one itemset
            if (alive) {
                if constexpr (W1) {
                    uint64_t acc = prev < 0 ? ~0ull : (prev >= 63 ? 0ull : (~0ull << (prev + 1)));
                    for (uint32_t q = i; q < j && acc; ++q) {
                        const uint32_t it = tok[q] & ~kPsOpen;
                        const uint32_t en = it == pv ? pent : ps_find(item, rb, re, it);
                        acc = en == kNone ? 0ull : (acc & mask[en]);
                    }
                    alive = acc != 0;
                    if (alive) prev = int32_t(__builtin_ctzll(acc));
                } else {
                    // the entries first (a miss retires the lane); the first kPsSetRegs stay in registers
                    uint32_t ent[kPsSetRegs];
#pragma unroll
                    for (int c = 0; c < kPsSetRegs; ++c) ent[c] = 0;
                    for (uint32_t q = i; q < j && alive; ++q) {
                        const uint32_t it = tok[q] & ~kPsOpen;
                        const uint32_t en = it == pv ? pent : ps_find(item, rb, re, it);
                        alive = en != kNone;
#pragma unroll
                        for (int c = 0; c < kPsSetRegs; ++c) ent[c] = (q - i == uint32_t(c)) ? en : ent[c];
                    }
                    if (alive) {
                        const uint32_t from = uint32_t(prev + 1);  // lowest eid allowed
                        uint64_t acc = 0;
                        uint32_t w = from >> 6;
                        for (; w < wd; ++w) {
                            acc = w == (from >> 6) ? (~0ull << (from & 63u)) : ~0ull;
#pragma unroll
                            for (int c = 0; c < kPsSetRegs; ++c)
                                if (i + uint32_t(c) < j) acc &= mask[uint64_t(ent[c]) * wd + w];
                            for (uint32_t q = i + kPsSetRegs; q < j && acc; ++q) {  // (found above: never kNone)
                                const uint32_t it = tok[q] & ~kPsOpen;
                                const uint32_t en = it == pv ? pent : ps_find(item, rb, re, it);
                                acc &= mask[uint64_t(en) * wd + w];
                            }
                            if (acc) break;
                        }
                        alive = acc != 0;
                        if (alive) prev = int32_t(w * 64 + uint32_t(__builtin_ctzll(acc)));
                    }
                }
            }
            i = j;
        }
        const uint64_t live = ballot(alive);
        if (live != 0 && lane_id() == 0) atomicAdd(&count[p], int32_t(__popcll(live)));
    }
}

unsigned ps_grid(uint64_t work, uint64_t per_block) {
    return unsigned(std::min<uint64_t>(std::max<uint64_t>((work + per_block - 1) / per_block, 1), kPsMaxGrid));
}

// The vertical index of the DB, made once (a later call finds vert_state == 1).
void ps_build_index(fsm_ctx* ctx, SpadeDevDB* d, KernelClock& clock) {
    if (d->vert_state == 1) return;
    hipStream_t s = ctx->stream;
    const size_t U = size_t(d->U), E = size_t(d->E), R = size_t(d->R);
    DevBuf vert_off((U + 1) * 4), vert(std::max<size_t>(E, 1) * 8);
    DevBuf cnt(std::max<size_t>(U, 1) * 4), off((U + 1) * 8), cursor((U + 1) * 4);
    std::vector<uint32_t> host(U + 1, 0);
    if (U && E) {
        FSM_HIP(hipMemsetAsync(cnt.p, 0, U * 4, s));
        size_t tk = clock.begin("k_ps_index_hist");
        hipLaunchKernelGGL(k_ps_index_hist, dim3(ps_grid(E, kPsBlock)), dim3(kPsBlock), 0, s, d->item.as<uint32_t>(),
                           uint32_t(E), cnt.as<uint32_t>());
        FSM_LAUNCHED("k_ps_index_hist", s);
        clock.end(tk, int64_t(E) * (4 + 4));  // item read, one counter bumped per entry
        scan_exclusive(cnt.as<uint32_t>(), off.as<uint64_t>(), U, s);
        tk = clock.begin("k_ps_index_off");
        hipLaunchKernelGGL(k_ps_index_off, dim3(ps_grid(U + 1, kPsBlock)), dim3(kPsBlock), 0, s, off.as<uint64_t>(),
                           uint32_t(U + 1), vert_off.as<uint32_t>(), cursor.as<uint32_t>());
        FSM_LAUNCHED("k_ps_index_off", s);
        clock.end(tk, int64_t(U + 1) * (8 + 4 + 4));  // offset read, narrowed twice
        tk = clock.begin("k_ps_index_scatter");
        hipLaunchKernelGGL(k_ps_index_scatter, dim3(ps_grid(R, kPsBlock / 64)), dim3(kPsBlock), 0, s,
                           d->row_off.as<uint32_t>(), d->item.as<uint32_t>(), uint32_t(R), cursor.as<uint32_t>(),
                           vert.as<uint2>());
        FSM_LAUNCHED("k_ps_index_scatter", s);
        // row bounds per row; per entry: item read, cursor bumped, (row, entry) written
        clock.end(tk, int64_t(R) * 8 + int64_t(E) * (4 + 4 + 8));
        FSM_HIP(hipMemcpyAsync(host.data(), vert_off.p, (U + 1) * 4, hipMemcpyDeviceToHost, s));
        FSM_HIP(hipStreamSynchronize(s));
        if (host[U] != uint32_t(E)) throw Error(FSM_EDEVICE, "fsm_patterns_support: the vertical index lost entries");
    }
    d->vert_off = std::move(vert_off);
    d->vert = std::move(vert);
    d->vert_off_host = std::move(host);
    d->vert_state = 1;
}

// FSM_PS_PIVOT=first|last (test hook, read once per call): the pattern's first / last item
// is its pivot whatever the list lengths; 0 = the shortest list
int ps_pivot_hook() {
    const char* v = std::getenv("FSM_PS_PIVOT");
    if (!v) return 0;
    if (!std::strcmp(v, "first")) return 1;
    if (!std::strcmp(v, "last")) return 2;
    return 0;
}

// FSM_PS_SLICE_TILES=k (test hook, read once per call): tiles per launch at most
uint64_t ps_slice_tiles() {
    const char* v = std::getenv("FSM_PS_SLICE_TILES");
    if (!v || !*v) return kPsSliceTiles;
    char* end = nullptr;
    const long long k = std::strtoll(v, &end, 10);
    if (end == v || *end || k < 1 || uint64_t(k) > kPsSliceTiles) return kPsSliceTiles;
    return uint64_t(k);
}

}  // namespace

void patterns_support(fsm_ctx* ctx, fsm_db* db, const fsm_patterns* in, int32_t* support_out) {
    const char* who = "fsm_patterns_support";
    const int64_t n = in->n, ni = in->n_items;
    if (n < 0 || in->n_sets < 0 || ni < 0) throw Error(FSM_EINVAL, std::string(who) + ": negative sizes");
    constexpr int64_t kLimit = (int64_t(1) << 32) - 2;
    if (n >= kLimit || ni >= kLimit) throw Error(FSM_ELIMIT, std::string(who) + ": 2^32 - 2 or more patterns or items");
    if (n == 0) {
        if (in->n_sets != 0 || ni != 0) throw Error(FSM_EINVAL, std::string(who) + ": itemsets or items without patterns");
        ctx->kstats.clear();
        return;
    }
    // (the upload sources: declared ahead of the stream guard, which outlives no queued copy)
    std::vector<uint32_t> ioff, tok, piv, toff;
    std::vector<uint8_t> start;
    pf_validate(in, who, false, ioff, start);
    const int pivot_hook = ps_pivot_hook();
    const uint64_t slice_tiles = ps_slice_tiles();

    // the input is valid: device work from here on (the index first: the pivots need its lengths)
    SpadeDevDB* d = db->spade_dev;
    if (d->U >= (int64_t(1) << 31)) throw Error(FSM_ELIMIT, std::string(who) + ": 2^31 or more distinct items in the DB");
    FSM_HIP(hipSetDevice(ctx->opts.device));
    hipStream_t s = ctx->stream;
    struct SyncOnExit {
        hipStream_t s;
        ~SyncOnExit() { (void)hipStreamSynchronize(s); }
    } sync_on_exit{s};
    KernelClock clock(s);
    ClockScope clock_scope(&clock);  // (the index build's scan records into it)
    ps_build_index(ctx, d, clock);

    // tokens (dense id | opens-an-itemset), pivots and tiles, split over the host threads by patterns
    const std::vector<int32_t>& val = db->spade.item_val;
    const uint32_t* vlen = d->vert_off_host.data();
    const int64_t max_sets = int64_t(64) * d->W;
    const size_t un = size_t(n), ui = size_t(ni);
    tok.resize(ui);
    piv.resize(un);
    std::vector<uint64_t> tile_off(un + 1, 0);  // tiles of pattern p at [p + 1], summed below
    const int64_t nthr = n >= 65536 ? host_threads() : 1;
    par_slices(nthr, n, [&](int64_t, int64_t a, int64_t b) {
        for (int64_t p = a; p < b; ++p) {
            const uint32_t i0 = ioff[size_t(p)], i1 = ioff[size_t(p) + 1];
            bool live = in->pat_off[p + 1] - in->pat_off[p] <= max_sets;
            uint32_t best = kPsDead, best_len = 0;
            for (uint32_t i = i0; i < i1; ++i) {
                const auto it = std::lower_bound(val.begin(), val.end(), in->items[i]);
                if (it == val.end() || *it != in->items[i]) {
                    live = false;
                    tok[i] = start[i] ? kPsOpen : 0;  // (never read: the pattern gets no tile)
                    continue;
                }
                const uint32_t id = uint32_t(it - val.begin());
                tok[i] = id | (start[i] ? kPsOpen : 0u);
                const uint32_t len = vlen[id + 1] - vlen[id];
                if (best == kPsDead || len < best_len) {
                    best = i;
                    best_len = len;
                }
            }
            if (live && pivot_hook) {
                best = pivot_hook == 1 ? i0 : i1 - 1;
                const uint32_t id = tok[best] & ~kPsOpen;
                best_len = vlen[id + 1] - vlen[id];
            }
            piv[size_t(p)] = live ? best : kPsDead;
            tile_off[size_t(p) + 1] = live ? (uint64_t(best_len) + kPsTile - 1) / kPsTile : 0;
        }
    });
    int64_t tests = 0, live_items = 0;  // (pattern, row) pairs and their pattern items, for the bytes
    for (size_t p = 0; p < un; ++p) {
        if (piv[p] != kPsDead) {
            const uint32_t id = tok[piv[p]] & ~kPsOpen;
            const int64_t len = vlen[id + 1] - vlen[id];
            tests += len;
            live_items += len * int64_t(ioff[p + 1] - ioff[p]);
        }
        tile_off[p + 1] += tile_off[p];
    }
    const uint64_t total_tiles = tile_off[un];

    DevBuf d_count(un * 4);
    FSM_HIP(hipMemsetAsync(d_count.p, 0, un * 4, s));
    if (total_tiles) {
        // launches of at most slice_tiles tiles over whole patterns (one pattern has fewer than
        // 2^26 tiles); toff is relative to its launch's first tile, so it fits 32 bits
        toff.resize(un);
        std::vector<std::pair<uint32_t, uint32_t>> slices;
        for (size_t a = 0; a < un;) {
            size_t b = a + 1;
            while (b < un && tile_off[b + 1] - tile_off[a] <= slice_tiles) ++b;
            for (size_t p = a; p < b; ++p) toff[p] = uint32_t(tile_off[p] - tile_off[a]);
            slices.emplace_back(uint32_t(a), uint32_t(b));
            a = b;
        }
        DevBuf d_tok(ui * 4), d_ioff((un + 1) * 4), d_piv(un * 4), d_toff(un * 4);
        FSM_HIP(hipMemcpyAsync(d_tok.p, tok.data(), ui * 4, hipMemcpyHostToDevice, s));
        FSM_HIP(hipMemcpyAsync(d_ioff.p, ioff.data(), (un + 1) * 4, hipMemcpyHostToDevice, s));
        FSM_HIP(hipMemcpyAsync(d_piv.p, piv.data(), un * 4, hipMemcpyHostToDevice, s));
        FSM_HIP(hipMemcpyAsync(d_toff.p, toff.data(), un * 4, hipMemcpyHostToDevice, s));
        const size_t tk = clock.begin("k_ps_count");
        for (const auto& sl : slices) {
            const uint64_t nt = tile_off[sl.second] - tile_off[sl.first];
            if (!nt) continue;
            const dim3 grid(ps_grid(nt, kPsBlock / kPsTile)), block(kPsBlock);
            if (d->W == 1)
                hipLaunchKernelGGL(k_ps_count<true>, grid, block, 0, s, d->row_off.as<uint32_t>(), d->item.as<uint32_t>(),
                                   d->mask.as<uint64_t>(), 1u, d->vert_off.as<uint32_t>(), d->vert.as<uint2>(),
                                   d_tok.as<uint32_t>(), d_ioff.as<uint32_t>(), d_piv.as<uint32_t>(),
                                   d_toff.as<uint32_t>(), sl.first, sl.second, nt, d_count.as<int32_t>());
            else
                hipLaunchKernelGGL(k_ps_count<false>, grid, block, 0, s, d->row_off.as<uint32_t>(), d->item.as<uint32_t>(),
                                   d->mask.as<uint64_t>(), uint32_t(d->W), d->vert_off.as<uint32_t>(),
                                   d->vert.as<uint2>(), d_tok.as<uint32_t>(), d_ioff.as<uint32_t>(),
                                   d_piv.as<uint32_t>(), d_toff.as<uint32_t>(), sl.first, sl.second, nt,
                                   d_count.as<int32_t>());
            FSM_LAUNCHED("k_ps_count", s);
        }
        // as if no lane retired early.  Per (pattern, row) test: the list entry (8) and the row
        // bounds (8); per pattern item of a test: one item word (the search's last probe, 4) and
        // one mask word (8).  Per tile: its pattern's offsets, pivot, tile offset and list bounds
        // (24) and one counter add (4)
        clock.end(tk, tests * 16 + live_items * 12 + int64_t(total_tiles) * 28);
        FSM_HIP(hipMemcpyAsync(support_out, d_count.p, un * 4, hipMemcpyDeviceToHost, s));
        clock.finish(ctx->kstats);  // synchronizes the stream
    } else {
        clock.finish(ctx->kstats);
        std::memset(support_out, 0, un * 4);
    }
}

}  // namespace fsm
