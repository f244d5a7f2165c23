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
//
// fsm_patterns_sids returns the rows behind the counts as sequence ids.  Same tiles, same walk
// (ps_walk, shared with the count), but every tile keeps its survivors, and no atomics:
//
//   k_ps_index_order    once per DB: every list in ascending row order (a radix sort of the
//                       DB entries by (item, entry index); vert_state 2)
//   k_ps_match          the count's pass; lane 0 writes the tile's ballot and its popcount
//   k_scan              fsm::scan_exclusive over the popcounts: the ids ahead of every tile
//   k_ps_pat_off        the scanned offsets at the patterns' first tiles: off[] and the total
//   k_ps_sids_write     a wave reads 64 tiles' ballots and offsets at once, then, one tile
//                       with survivors at a time, the set lanes write their row's sequence id
//                       at the tile's offset plus their rank in the ballot; in slices of whole
//                       patterns through a staging buffer of kPsSliceSids ids
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
constexpr uint64_t kPsSliceSids = 16777216;  // ids per write slice at most: a 64 MiB staging buffer

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

// The containment walk both passes share: does the row of entry rel * kPsTile + lane of
// pattern p's pivot list contain p?  (p and rel are wave-uniform; every lane of the wave
// calls it.)  W1: one-word masks (the AND stays in a register); otherwise `wd` words per
// mask, walked from the previous eid's word on.
template <bool W1>
__device__ __forceinline__ bool ps_walk(const uint32_t* __restrict__ row_off, const uint32_t* __restrict__ item,
                                        const uint64_t* __restrict__ mask, uint32_t wd,
                                        const uint32_t* __restrict__ vert_off, const uint2* __restrict__ vert,
                                        const uint32_t* __restrict__ tok, const uint32_t* __restrict__ ioff,
                                        const uint32_t* __restrict__ piv, uint32_t p, uint32_t rel) {
    const uint32_t ib = ioff[p], ie = ioff[p + 1];
    const uint32_t pv = tok[piv[p]] & ~kPsOpen;  // the pivot's dense id
    const uint32_t lb = vert_off[pv], ln = vert_off[pv + 1] - lb;
    const uint32_t k = rel * kPsTile + lane_id();
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
    return alive;
}

// the pattern of tile t: the last p of [p0, p1) with toff[p] <= t
__device__ __forceinline__ uint32_t ps_tile_pattern(const uint32_t* __restrict__ toff, uint32_t p0, uint32_t p1,
                                                    uint32_t t) {
    uint32_t lo = p0, hi = p1;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (toff[mid] <= t) lo = mid;
        else hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// Tile t (relative to this launch's first tile) belongs to the last pattern p of [p0, p1)
// with toff[p] <= t; toff[p0] = 0 and patterns without tiles repeat their successor's value.
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
        const uint32_t p = ps_tile_pattern(toff, p0, p1, t);
        const bool alive = ps_walk<W1>(row_off, item, mask, wd, vert_off, vert, tok, ioff, piv, p, t - toff[p]);
        const uint64_t live = ballot(alive);
        if (live != 0 && lane_id() == 0) atomicAdd(&count[p], int32_t(__popcll(live)));
    }
}

// ---------------------------------------------------------------- sequence ids
// The count's tiles and walk; every tile keeps its survivors: their ballot in live[t] and its
// popcount in tcnt[t] (both relative to this launch's first tile), zero ballots included.
template <bool W1>
__global__ __launch_bounds__(kPsBlock) void k_ps_match(const uint32_t* __restrict__ row_off,
                                                       const uint32_t* __restrict__ item,
                                                       const uint64_t* __restrict__ mask, uint32_t wd,
                                                       const uint32_t* __restrict__ vert_off,
                                                       const uint2* __restrict__ vert,
                                                       const uint32_t* __restrict__ tok,
                                                       const uint32_t* __restrict__ ioff,
                                                       const uint32_t* __restrict__ piv,
                                                       const uint32_t* __restrict__ toff, uint32_t p0, uint32_t p1,
                                                       uint64_t ntiles, uint64_t* __restrict__ live_out,
                                                       uint32_t* __restrict__ tcnt) {
    const uint64_t waves = uint64_t(gridDim.x) * (kPsBlock / kPsTile);
    for (uint64_t t64 = uint64_t(blockIdx.x) * (kPsBlock / kPsTile) + threadIdx.x / kPsTile; t64 < ntiles; t64 += waves) {
        const uint32_t t = uint32_t(t64);
        const uint32_t p = ps_tile_pattern(toff, p0, p1, t);
        const bool alive = ps_walk<W1>(row_off, item, mask, wd, vert_off, vert, tok, ioff, piv, p, t - toff[p]);
        const uint64_t live = ballot(alive);
        if (lane_id() == 0) {
            live_out[t64] = live;
            tcnt[t64] = uint32_t(__popcll(live));
        }
    }
}

// poff[p] = ids ahead of pattern p = the scanned offset of its first tile (tile_off[n] is the
// tile total, tsum's last entry the id total)
__global__ __launch_bounds__(kPsBlock) void k_ps_pat_off(const uint64_t* __restrict__ tile_off,
                                                         const uint64_t* __restrict__ tsum, uint64_t n1,
                                                         uint64_t* __restrict__ poff) {
    const uint64_t stride = uint64_t(gridDim.x) * kPsBlock;
    for (uint64_t p = uint64_t(blockIdx.x) * kPsBlock + threadIdx.x; p < n1; p += stride) poff[p] = tsum[tile_off[p]];
}

// The tiles [t0, t0 + ntiles) of the call belong to the patterns [p0, p1).  A wave takes 64
// consecutive tiles: every lane reads one tile's ballot and offset (coalesced; most tiles of a
// mined set are empty, and a wave that read one ballot per step would wait a memory latency
// for each), then the wave handles the tiles with survivors one at a time: the lanes whose bit
// is set in the tile's ballot write the sequence id of their row at the tile's offset plus
// their rank among the set bits: contiguous 4-byte stores, in list order.  `base` = ids ahead
// of pattern p0 (out starts there).
__global__ __launch_bounds__(kPsBlock) void k_ps_sids_write(const uint64_t* __restrict__ tile_off, uint32_t p0,
                                                            uint32_t p1, uint64_t t0, uint64_t ntiles,
                                                            const uint64_t* __restrict__ live_in,
                                                            const uint64_t* __restrict__ tsum, uint64_t base,
                                                            const uint32_t* __restrict__ vert_off,
                                                            const uint2* __restrict__ vert,
                                                            const uint32_t* __restrict__ tok,
                                                            const uint32_t* __restrict__ piv,
                                                            const int32_t* __restrict__ row_sid,
                                                            int32_t* __restrict__ out) {
    const uint64_t waves = uint64_t(gridDim.x) * (kPsBlock / kPsTile);
    const uint64_t chunks = (ntiles + kPsTile - 1) / kPsTile;
    for (uint64_t c = uint64_t(blockIdx.x) * (kPsBlock / kPsTile) + threadIdx.x / kPsTile; c < chunks; c += waves) {
        const uint64_t i = c * kPsTile + lane_id();
        uint64_t mine = 0, at = 0;
        if (i < ntiles) {
            mine = live_in[t0 + i];
            at = tsum[t0 + i];
        }
        uint64_t todo = ballot(mine != 0);
        uint32_t p = p0;
        uint64_t pend = 0;  // the tiles of p end here (0: no pattern looked up yet; the tiles ascend)
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t live = __shfl(mine, j, 64), off = __shfl(at, j, 64);
            const uint64_t t = t0 + c * kPsTile + uint64_t(j);
            if (t >= pend) {  // the last pattern of [p0, p1) with tile_off[p] <= t
                uint32_t lo = p0, hi = p1;
                while (hi - lo > 1) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (tile_off[mid] <= t) lo = mid;
                    else hi = mid;
                }
                p = __builtin_amdgcn_readfirstlane(lo);
                pend = tile_off[p + 1];
            }
            const uint32_t pv = tok[piv[p]] & ~kPsOpen;
            const uint32_t k = uint32_t(t - tile_off[p]) * kPsTile + lane_id();
            if ((live >> lane_id()) & 1ull)  // (set only for k inside the list)
                out[off - base + uint64_t(__popcll(live & lanemask_lt()))] = row_sid[vert[vert_off[pv] + k].x];
        }
    }
}

// ---------------------------------------------------------------- list order
// keys of the ordering sort: dense item id << 32 | entry index (entry indexes ascend with rows)
__global__ __launch_bounds__(kPsBlock) void k_ps_order_keys(const uint32_t* __restrict__ item, uint32_t E,
                                                            uint64_t* __restrict__ keys) {
    const uint64_t stride = uint64_t(gridDim.x) * kPsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kPsBlock + threadIdx.x; i < E; i += stride)
        keys[i] = (uint64_t(item[i]) << 32) | i;
}

// the sorted keys are the vertical lists back to back in ascending entry order: slot i gets
// (row of the entry, entry); the row is the last r with row_off[r] <= entry
__global__ __launch_bounds__(kPsBlock) void k_ps_order_rows(const uint64_t* __restrict__ sorted, uint32_t E,
                                                            const uint32_t* __restrict__ row_off, uint32_t R,
                                                            uint2* __restrict__ vert) {
    const uint64_t stride = uint64_t(gridDim.x) * kPsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kPsBlock + threadIdx.x; i < E; i += stride) {
        const uint32_t ent = uint32_t(sorted[i]);
        uint32_t lo = 0, hi = R;  // (R >= 1 when E >= 1)
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (row_off[mid] <= ent) lo = mid;
            else hi = mid;
        }
        vert[i] = make_uint2(lo, ent);
    }
}

unsigned ps_grid(uint64_t work, uint64_t per_block) {
    return unsigned(std::min<uint64_t>(std::max<uint64_t>((work + per_block - 1) / per_block, 1), kPsMaxGrid));
}

// The vertical index of the DB, made once (a later call finds vert_state == 1).
void ps_build_index(fsm_ctx* ctx, SpadeDevDB* d, KernelClock& clock) {
    if (d->vert_state >= 1) return;
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


// The lists of the vertical index in ascending row order, once per DB (vert_state 2): the
// DB entries sorted by (dense item id, entry index).  The keys are distinct, so the result
// does not rest on the sort being stable, and it falls into the slots of vert_off as they are.
void ps_order_index(fsm_ctx* ctx, SpadeDevDB* d, KernelClock& clock) {
    if (d->vert_state == 2) return;
    hipStream_t s = ctx->stream;
    const size_t U = size_t(d->U), E = size_t(d->E), R = size_t(d->R);
    if (U && E) {
        DevBuf keys(E * 8), sorted(E * 8);
        unsigned item_bits = 1;
        while (item_bits < 32 && (uint64_t(1) << item_bits) < U) ++item_bits;
        const size_t tk = clock.begin("k_ps_index_order");
        hipLaunchKernelGGL(k_ps_order_keys, dim3(ps_grid(E, kPsBlock)), dim3(kPsBlock), 0, s, d->item.as<uint32_t>(),
                           uint32_t(E), keys.as<uint64_t>());
        FSM_LAUNCHED("k_ps_order_keys", s);
        sort_entry_keys(keys.as<uint64_t>(), sorted.as<uint64_t>(), E, item_bits, s);
        hipLaunchKernelGGL(k_ps_order_rows, dim3(ps_grid(E, kPsBlock)), dim3(kPsBlock), 0, s, sorted.as<uint64_t>(),
                           uint32_t(E), d->row_off.as<uint32_t>(), uint32_t(R), d->vert.as<uint2>());
        FSM_LAUNCHED("k_ps_order_rows", s);
        // per entry: item read and key written (12); one read and one write of the key per
        // 8-bit digit pass of the sort (16 each); the sorted key, the search's last probe and
        // the list entry (20)
        const int64_t passes = (32 + int64_t(item_bits) + 7) / 8;
        clock.end(tk, int64_t(E) * (12 + 16 * passes + 20));
        FSM_HIP(hipStreamSynchronize(s));  // (keys and sorted are released here)
    }
    d->vert_state = 2;
}

// the device copy of the rows' sequence ids, made once per DB
void ps_upload_row_sids(fsm_ctx* ctx, const fsm_db* db, SpadeDevDB* d) {
    if (d->row_sid_made) return;
    if (int64_t(db->row_sid.size()) != d->R)
        throw Error(FSM_EDEVICE, "fsm_patterns_sids: the DB has " + std::to_string(d->R) + " rows and " +
                                     std::to_string(db->row_sid.size()) + " sequence ids");
    DevBuf dev(std::max<size_t>(size_t(d->R), 1) * 4);
    if (d->R) {
        FSM_HIP(hipMemcpyAsync(dev.p, db->row_sid.data(), size_t(d->R) * 4, hipMemcpyHostToDevice, ctx->stream));
        FSM_HIP(hipStreamSynchronize(ctx->stream));
    }
    d->row_sid = std::move(dev);
    d->row_sid_made = true;
}

// The test hooks, read once per call into one snapshot:
//   FSM_PS_PIVOT=first|last  the pattern's first / last item is its pivot whatever the list
//                            lengths; 0 = the shortest list
//   FSM_PS_SLICE_TILES=k     tiles per launch at most
//   FSM_PS_SLICE_SIDS=k      fsm_patterns_sids: ids per write slice at most
struct PsHooks {
    int pivot = 0;
    uint64_t slice_tiles = kPsSliceTiles;
    uint64_t slice_sids = kPsSliceSids;
};

uint64_t ps_env_count(const char* name, uint64_t dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    char* end = nullptr;
    const long long k = std::strtoll(v, &end, 10);
    if (end == v || *end || k < 1 || uint64_t(k) > dflt) return dflt;
    return uint64_t(k);
}

PsHooks ps_hooks() {
    PsHooks h;
    if (const char* v = std::getenv("FSM_PS_PIVOT")) h.pivot = !std::strcmp(v, "first") ? 1 : (!std::strcmp(v, "last") ? 2 : 0);
    h.slice_tiles = ps_env_count("FSM_PS_SLICE_TILES", kPsSliceTiles);
    h.slice_sids = ps_env_count("FSM_PS_SLICE_SIDS", kPsSliceSids);
    return h;
}

// the size checks ahead of pf_validate; false: no patterns (nothing to do)
bool ps_check_sizes(const fsm_patterns* in, const char* who) {
    const int64_t n = in->n, ni = in->n_items;
    if (n < 0 || in->n_sets < 0 || ni < 0) throw Error(FSM_EINVAL, std::string(who) + ": negative sizes");
    constexpr int64_t kLimit = (int64_t(1) << 32) - 2;
    if (n >= kLimit || ni >= kLimit) throw Error(FSM_ELIMIT, std::string(who) + ": 2^32 - 2 or more patterns or items");
    if (n == 0 && (in->n_sets != 0 || ni != 0))
        throw Error(FSM_EINVAL, std::string(who) + ": itemsets or items without patterns");
    return n != 0;
}

// What a call's tile launches read.  The vectors are the sources of queued uploads: a plan is
// declared ahead of the call's stream guard, which outlives no queued copy.
struct PsPlan {
    std::vector<uint32_t> ioff, tok, piv, toff;
    std::vector<uint8_t> start;
    std::vector<uint64_t> tile_off;  // [n + 1] first tile of every pattern, of the whole call
    std::vector<std::pair<uint32_t, uint32_t>> slices;  // launches: whole patterns [first, second)
    int64_t tests = 0, live_items = 0;  // (pattern, row) pairs and their pattern items, for the bytes
    uint64_t total_tiles = 0;
    DevBuf d_tok, d_ioff, d_piv, d_toff;
    // as if no lane retired early.  Per (pattern, row) test: the list entry (8) and the row
    // bounds (8); per pattern item of a test: one item word (the search's last probe, 4) and
    // one mask word (8).  Per tile: its pattern's offsets, pivot, tile offset and list bounds
    // (24) and what the pass writes (`out`: one counter add, 4; a ballot and its popcount, 12)
    int64_t walk_bytes(int64_t out) const { return tests * 16 + live_items * 12 + int64_t(total_tiles) * (24 + out); }
};

struct PsSyncOnExit {
    hipStream_t s;
    ~PsSyncOnExit() { (void)hipStreamSynchronize(s); }
};

// tokens (dense id | opens-an-itemset), pivots and tiles of validated patterns (ioff and start
// filled by pf_validate), split over the host threads by patterns; the index is built
void ps_plan(const fsm_db* db, const SpadeDevDB* d, const fsm_patterns* in, const PsHooks& hk, PsPlan& pl) {
    const int64_t n = in->n;
    const std::vector<int32_t>& val = db->spade.item_val;
    const uint32_t* vlen = d->vert_off_host.data();
    const int64_t max_sets = int64_t(64) * d->W;
    const size_t un = size_t(n), ui = size_t(in->n_items);
    const std::vector<uint32_t>& ioff = pl.ioff;
    const std::vector<uint8_t>& start = pl.start;
    std::vector<uint32_t>& tok = pl.tok;
    std::vector<uint32_t>& piv = pl.piv;
    std::vector<uint64_t>& tile_off = pl.tile_off;
    tok.resize(ui);
    piv.resize(un);
    tile_off.assign(un + 1, 0);  // tiles of pattern p at [p + 1], summed below
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
            if (live && hk.pivot) {
                best = hk.pivot == 1 ? i0 : i1 - 1;
                const uint32_t id = tok[best] & ~kPsOpen;
                best_len = vlen[id + 1] - vlen[id];
            }
            piv[size_t(p)] = live ? best : kPsDead;
            tile_off[size_t(p) + 1] = live ? (uint64_t(best_len) + kPsTile - 1) / kPsTile : 0;
        }
    });
    for (size_t p = 0; p < un; ++p) {
        if (piv[p] != kPsDead) {
            const uint32_t id = tok[piv[p]] & ~kPsOpen;
            const int64_t len = vlen[id + 1] - vlen[id];
            pl.tests += len;
            pl.live_items += len * int64_t(ioff[p + 1] - ioff[p]);
        }
        tile_off[p + 1] += tile_off[p];
    }
    pl.total_tiles = tile_off[un];
}

// launches of at most slice_tiles tiles over whole patterns (one pattern has fewer than 2^26
// tiles); toff is relative to its launch's first tile, so it fits 32 bits.  Queues the uploads.
void ps_upload(PsPlan& pl, const PsHooks& hk, hipStream_t s) {
    const size_t un = pl.piv.size(), ui = pl.tok.size();
    const std::vector<uint64_t>& tile_off = pl.tile_off;
    pl.toff.resize(un);
    for (size_t a = 0; a < un;) {
        size_t b = a + 1;
        while (b < un && tile_off[b + 1] - tile_off[a] <= hk.slice_tiles) ++b;
        for (size_t p = a; p < b; ++p) pl.toff[p] = uint32_t(tile_off[p] - tile_off[a]);
        pl.slices.emplace_back(uint32_t(a), uint32_t(b));
        a = b;
    }
    pl.d_tok.alloc(ui * 4);
    pl.d_ioff.alloc((un + 1) * 4);
    pl.d_piv.alloc(un * 4);
    pl.d_toff.alloc(un * 4);
    FSM_HIP(hipMemcpyAsync(pl.d_tok.p, pl.tok.data(), ui * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(pl.d_ioff.p, pl.ioff.data(), (un + 1) * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(pl.d_piv.p, pl.piv.data(), un * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(pl.d_toff.p, pl.toff.data(), un * 4, hipMemcpyHostToDevice, s));
}

// launch(W1 tag, grid, wd, first pattern, last pattern, first tile of the call, tiles) per slice
template <class F> void ps_for_slices(const PsPlan& pl, F&& launch) {
    for (const auto& sl : pl.slices) {
        const uint64_t nt = pl.tile_off[sl.second] - pl.tile_off[sl.first];
        if (nt) launch(dim3(ps_grid(nt, kPsBlock / kPsTile)), sl.first, sl.second, pl.tile_off[sl.first], nt);
    }
}

}  // namespace

void patterns_support(fsm_ctx* ctx, fsm_db* db, const fsm_patterns* in, int32_t* support_out) {
    const char* who = "fsm_patterns_support";
    if (!ps_check_sizes(in, who)) {
        ctx->kstats.clear();
        return;
    }
    PsPlan pl;
    pf_validate(in, who, false, pl.ioff, pl.start);
    const PsHooks hk = ps_hooks();

    // the input is valid: device work from here on (the index first: the pivots need its lengths)
    SpadeDevDB* d = db->spade_dev;
    if (d->U >= (int64_t(1) << 31)) throw Error(FSM_ELIMIT, std::string(who) + ": 2^31 or more distinct items in the DB");
    FSM_HIP(hipSetDevice(ctx->opts.device));
    hipStream_t s = ctx->stream;
    PsSyncOnExit sync_on_exit{s};
    KernelClock clock(s);
    ClockScope clock_scope(&clock);  // (the index build's scan records into it)
    ps_build_index(ctx, d, clock);
    ps_plan(db, d, in, hk, pl);

    const size_t un = size_t(in->n);
    DevBuf d_count(un * 4);
    FSM_HIP(hipMemsetAsync(d_count.p, 0, un * 4, s));
    if (pl.total_tiles) {
        ps_upload(pl, hk, s);
        const size_t tk = clock.begin("k_ps_count");
        ps_for_slices(pl, [&](dim3 grid, uint32_t p0, uint32_t p1, uint64_t, uint64_t nt) {
            const dim3 block(kPsBlock);
            if (d->W == 1)
                hipLaunchKernelGGL(k_ps_count<true>, grid, block, 0, s, d->row_off.as<uint32_t>(), d->item.as<uint32_t>(),
                                   d->mask.as<uint64_t>(), 1u, d->vert_off.as<uint32_t>(), d->vert.as<uint2>(),
                                   pl.d_tok.as<uint32_t>(), pl.d_ioff.as<uint32_t>(), pl.d_piv.as<uint32_t>(),
                                   pl.d_toff.as<uint32_t>(), p0, p1, nt, d_count.as<int32_t>());
            else
                hipLaunchKernelGGL(k_ps_count<false>, grid, block, 0, s, d->row_off.as<uint32_t>(), d->item.as<uint32_t>(),
                                   d->mask.as<uint64_t>(), uint32_t(d->W), d->vert_off.as<uint32_t>(),
                                   d->vert.as<uint2>(), pl.d_tok.as<uint32_t>(), pl.d_ioff.as<uint32_t>(),
                                   pl.d_piv.as<uint32_t>(), pl.d_toff.as<uint32_t>(), p0, p1, nt,
                                   d_count.as<int32_t>());
            FSM_LAUNCHED("k_ps_count", s);
        });
        clock.end(tk, pl.walk_bytes(4));
        FSM_HIP(hipMemcpyAsync(support_out, d_count.p, un * 4, hipMemcpyDeviceToHost, s));
        clock.finish(ctx->kstats);  // synchronizes the stream
    } else {
        clock.finish(ctx->kstats);
        std::memset(support_out, 0, un * 4);
    }
}

void patterns_sids(fsm_ctx* ctx, fsm_db* db, const fsm_patterns* in, int64_t max_sids, fsm_sidlists** out) {
    const char* who = "fsm_patterns_sids";
    const bool any = ps_check_sizes(in, who);
    const size_t un = size_t(in->n);
    PsPlan pl;
    std::vector<uint64_t> poff;  // ids ahead of every pattern (read back; ahead of the stream guard)
    MallocArr<int64_t> r_off;
    MallocArr<int32_t> r_sid;
    auto result = [&](uint64_t total) {  // the library-owned struct; the arrays are released into it
        auto* r = static_cast<fsm_sidlists*>(std::calloc(1, sizeof(fsm_sidlists)));
        if (!r) throw Error(FSM_ENOMEM, "calloc failed");
        r->n = int64_t(un);
        r->n_sids = int64_t(total);
        r->off = r_off.release();
        r->sid = r_sid.release();
        *out = r;
    };
    if (!any) {
        r_off.alloc(1);
        r_sid.alloc(0);
        r_off[0] = 0;
        ctx->kstats.clear();
        result(0);
        return;
    }
    pf_validate(in, who, false, pl.ioff, pl.start);
    const PsHooks hk = ps_hooks();
    poff.assign(un + 1, 0);

    SpadeDevDB* d = db->spade_dev;
    if (d->U >= (int64_t(1) << 31)) throw Error(FSM_ELIMIT, std::string(who) + ": 2^31 or more distinct items in the DB");
    FSM_HIP(hipSetDevice(ctx->opts.device));
    hipStream_t s = ctx->stream;
    PsSyncOnExit sync_on_exit{s};
    KernelClock clock(s);
    ClockScope clock_scope(&clock);  // (the scans record into it)
    ps_build_index(ctx, d, clock);
    ps_order_index(ctx, d, clock);
    ps_upload_row_sids(ctx, db, d);
    ps_plan(db, d, in, hk, pl);

    // the match pass over every tile of the call, then the ids ahead of every tile and pattern
    const uint64_t TT = pl.total_tiles;
    DevBuf d_live, d_tcnt, d_tsum, d_tile_off, d_poff;
    if (TT) {
        ps_upload(pl, hk, s);
        d_live.alloc(TT * 8);
        d_tcnt.alloc(TT * 4);
        d_tsum.alloc((TT + 1) * 8);
        d_tile_off.alloc((un + 1) * 8);
        d_poff.alloc((un + 1) * 8);
        FSM_HIP(hipMemcpyAsync(d_tile_off.p, pl.tile_off.data(), (un + 1) * 8, hipMemcpyHostToDevice, s));
        const size_t tk = clock.begin("k_ps_match");
        ps_for_slices(pl, [&](dim3 grid, uint32_t p0, uint32_t p1, uint64_t t0, uint64_t nt) {
            const dim3 block(kPsBlock);
            if (d->W == 1)
                hipLaunchKernelGGL(k_ps_match<true>, grid, block, 0, s, d->row_off.as<uint32_t>(), d->item.as<uint32_t>(),
                                   d->mask.as<uint64_t>(), 1u, d->vert_off.as<uint32_t>(), d->vert.as<uint2>(),
                                   pl.d_tok.as<uint32_t>(), pl.d_ioff.as<uint32_t>(), pl.d_piv.as<uint32_t>(),
                                   pl.d_toff.as<uint32_t>(), p0, p1, nt, d_live.as<uint64_t>() + t0,
                                   d_tcnt.as<uint32_t>() + t0);
            else
                hipLaunchKernelGGL(k_ps_match<false>, grid, block, 0, s, d->row_off.as<uint32_t>(), d->item.as<uint32_t>(),
                                   d->mask.as<uint64_t>(), uint32_t(d->W), d->vert_off.as<uint32_t>(),
                                   d->vert.as<uint2>(), pl.d_tok.as<uint32_t>(), pl.d_ioff.as<uint32_t>(),
                                   pl.d_piv.as<uint32_t>(), pl.d_toff.as<uint32_t>(), p0, p1, nt,
                                   d_live.as<uint64_t>() + t0, d_tcnt.as<uint32_t>() + t0);
            FSM_LAUNCHED("k_ps_match", s);
        });
        clock.end(tk, pl.walk_bytes(12));
        scan_exclusive(d_tcnt.as<uint32_t>(), d_tsum.as<uint64_t>(), size_t(TT), s);
        // (a gather of n + 1 offsets, 24 bytes each: no row of its own in the statistics)
        hipLaunchKernelGGL(k_ps_pat_off, dim3(ps_grid(un + 1, kPsBlock)), dim3(kPsBlock), 0, s,
                           d_tile_off.as<uint64_t>(), d_tsum.as<uint64_t>(), uint64_t(un + 1), d_poff.as<uint64_t>());
        FSM_LAUNCHED("k_ps_pat_off", s);
        FSM_HIP(hipMemcpyAsync(poff.data(), d_poff.p, (un + 1) * 8, hipMemcpyDeviceToHost, s));
        FSM_HIP(hipStreamSynchronize(s));
    }
    const uint64_t total = poff[un];
    if (max_sids > 0 && total > uint64_t(max_sids))
        throw Error(FSM_ELIMIT, std::string(who) + ": the patterns have " + std::to_string(total) +
                                    " sequence ids in all, max_sids is " + std::to_string(max_sids));
    r_off.alloc(un + 1);
    r_sid.alloc(size_t(total));
    for (size_t p = 0; p <= un; ++p) r_off[p] = int64_t(poff[p]);

    if (total) {
        // the write in slices of whole patterns whose ids fit the staging buffer (a pattern with
        // more ids than slice_sids is a slice of its own), each copied to the result at its off
        uint64_t cap = 0;
        std::vector<std::pair<uint32_t, uint32_t>> wsl;
        for (size_t a = 0; a < un;) {
            size_t b = a + 1;
            while (b < un && poff[b + 1] - poff[a] <= hk.slice_sids) ++b;
            if (poff[b] > poff[a]) {
                wsl.emplace_back(uint32_t(a), uint32_t(b));
                cap = std::max(cap, poff[b] - poff[a]);
            }
            a = b;
        }
        DevBuf stage(size_t(cap) * 4);
        for (const auto& sl : wsl) {
            const uint64_t t0 = pl.tile_off[sl.first], nt = pl.tile_off[sl.second] - t0;
            const uint64_t base = poff[sl.first], ids = poff[sl.second] - base;
            const size_t tk = clock.begin("k_ps_sids_write");  // (the copies stay outside its events)
            hipLaunchKernelGGL(k_ps_sids_write, dim3(ps_grid(nt, kPsBlock)), dim3(kPsBlock), 0, s,
                               d_tile_off.as<uint64_t>(), sl.first, sl.second, t0, nt, d_live.as<uint64_t>(),
                               d_tsum.as<uint64_t>(), base, d->vert_off.as<uint32_t>(), d->vert.as<uint2>(),
                               pl.d_tok.as<uint32_t>(), pl.d_piv.as<uint32_t>(), d->row_sid.as<int32_t>(),
                               stage.as<int32_t>());
            FSM_LAUNCHED("k_ps_sids_write", s);
            // per tile: its ballot and its offset (16); per id: the list entry, the row's id, the store (12)
            clock.end(tk, int64_t(nt) * 16 + int64_t(ids) * 12);
            FSM_HIP(hipMemcpyAsync(r_sid.p + base, stage.p, size_t(ids) * 4, hipMemcpyDeviceToHost, s));
        }
    }
    clock.finish(ctx->kstats);  // synchronizes the stream
    result(total);
}

}  // namespace fsm
