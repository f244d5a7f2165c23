// pattern_filter.hip — closed / maximal filters over a complete frequent set
// (fsm_patterns_filter).
//
// Support is anti-monotone and the set is complete, so a pattern P has a strict
// super-pattern (of equal support, for closed) in the set iff some pattern Q of the
// set with exactly one item more yields P when one of its items is deleted (an
// itemset that becomes empty disappears; its neighbours are never merged).  That
// turns the quadratic containment search into a hash join over the sum of |Q|
// one-item deletions:
//
//   k_pf_hash    one thread per pattern: the polynomial hash sum h(token_k) * B^k of its
//                token stream (token = item, starts-a-new-itemset), every item's prefix
//                hash and owning pattern
//   k_pf_insert  the patterns' indexes into an open-addressed u32 table (atomicCAS,
//                linear probing, >= 2n slots)
//   k_pf_probe   one work item per flat item index = one (Q, deleted position): the
//                hash of Q minus that item from the prefix hashes in O(1), the chain
//                walk, and on every equal hash the exact check (item count, support for
//                closed, token by token) before drop[P] = 1 (a set-only store)
//
// A hash match alone never drops a pattern, so the result is exact whatever the hash
// does: FSM_PF_HASH_BITS=k (test hook) keeps only the low k bits of every hash.
// The kept patterns are compacted on the host (input order), where the caller's
// arrays and the result live.
#include <cstdio>
#include <cstring>

#include "device_util.h"
#include "host_pool.h"

namespace fsm {

namespace {

constexpr int kPfBlock = 256;
constexpr unsigned kPfMaxGrid = 8192;
constexpr uint32_t kPfEmpty = 0xFFFFFFFFu;
constexpr uint64_t kPfB = 0x9E3779B97F4A7C15ull;   // odd: invertible mod 2^64
constexpr uint64_t kPfLenK = 0xC2B2AE3D27D4EB4Full;
constexpr uint64_t kPfSupK = 0x165667B19E3779F9ull;

__host__ __device__ __forceinline__ uint64_t pf_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// hash of one token: the item (any int32) and whether it opens an itemset
__device__ __forceinline__ uint64_t pf_token(int32_t item, uint32_t start) {
    return pf_mix(((uint64_t(uint32_t(item)) << 1) | uint64_t(start & 1u)) + kPfB);
}

// the key's hash: token stream, item count and (closed) the support
__device__ __forceinline__ uint64_t pf_final(uint64_t raw, uint32_t len, int32_t sup, int closed, uint64_t hmask) {
    uint64_t x = raw + kPfLenK * uint64_t(len);
    if (closed) x += kPfSupK * uint64_t(uint32_t(sup));
    return pf_mix(x) & hmask;
}

__device__ __forceinline__ uint64_t pf_pow(uint32_t e) {  // B^e mod 2^64
    uint64_t r = 1, b = kPfB;
    for (; e; e >>= 1) {
        if (e & 1u) r *= b;
        b *= b;
    }
    return r;
}

// pattern p: items [ioff[p], ioff[p+1]); start[i] = 1 when item i opens an itemset
__global__ __launch_bounds__(kPfBlock) void k_pf_hash(const int32_t* __restrict__ items,
                                                      const uint8_t* __restrict__ start,
                                                      const uint32_t* __restrict__ ioff,
                                                      const int32_t* __restrict__ sup, uint32_t n, int closed,
                                                      uint64_t hmask, uint64_t* __restrict__ pre,
                                                      uint32_t* __restrict__ pid, uint64_t* __restrict__ raw,
                                                      uint64_t* __restrict__ hash) {
    const uint64_t stride = uint64_t(gridDim.x) * kPfBlock;
    for (uint64_t p = uint64_t(blockIdx.x) * kPfBlock + threadIdx.x; p < n; p += stride) {
        const uint32_t b = ioff[p], e = ioff[p + 1];
        uint64_t acc = 0, pw = 1;
        for (uint32_t i = b; i < e; ++i) {
            pre[i] = acc;
            pid[i] = uint32_t(p);
            acc += pf_token(items[i], start[i]) * pw;
            pw *= kPfB;
        }
        raw[p] = acc;
        hash[p] = pf_final(acc, e - b, sup[p], closed, hmask);
    }
}

// (the table has at least 2n slots, so a free one always exists)
__global__ __launch_bounds__(kPfBlock) void k_pf_insert(const uint64_t* __restrict__ hash, uint32_t n,
                                                        uint32_t* __restrict__ table, uint64_t tmask) {
    const uint64_t stride = uint64_t(gridDim.x) * kPfBlock;
    for (uint64_t p = uint64_t(blockIdx.x) * kPfBlock + threadIdx.x; p < n; p += stride) {
        uint64_t slot = hash[p] & tmask;
        while (atomicCAS(&table[slot], kPfEmpty, uint32_t(p)) != kPfEmpty) slot = (slot + 1) & tmask;
    }
}

// is pattern P exactly Q (items [qb, qb + len + 1)) without its item at qb + j ?
__device__ __forceinline__ bool pf_same(const int32_t* __restrict__ items, const uint8_t* __restrict__ start,
                                        uint32_t pb, uint32_t qb, uint32_t j, uint32_t len) {
    const uint32_t del_start = start[qb + j];
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t q = qb + (k < j ? k : k + 1);
        if (items[pb + k] != items[q]) return false;
        // the item after a deleted itemset opener opens the itemset in its place
        const uint32_t st = k == j ? uint32_t(start[q]) | del_start : uint32_t(start[q]);
        if (uint32_t(start[pb + k]) != st) return false;
    }
    return true;
}

__global__ __launch_bounds__(kPfBlock) void k_pf_probe(const int32_t* __restrict__ items,
                                                       const uint8_t* __restrict__ start,
                                                       const uint32_t* __restrict__ ioff,
                                                       const int32_t* __restrict__ sup,
                                                       const uint64_t* __restrict__ pre,
                                                       const uint32_t* __restrict__ pid,
                                                       const uint64_t* __restrict__ raw,
                                                       const uint64_t* __restrict__ hash,
                                                       const uint32_t* __restrict__ table, uint64_t tmask,
                                                       uint64_t n_items, int closed, uint64_t hmask, uint64_t binv,
                                                       uint8_t* __restrict__ drop) {
    const uint64_t stride = uint64_t(gridDim.x) * kPfBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kPfBlock + threadIdx.x; i < n_items; i += stride) {
        const uint32_t q = pid[i];
        const uint32_t b = ioff[q], e = ioff[q + 1];
        const uint32_t len = e - b - 1;  // items of Q minus one
        if (len == 0) continue;          // a 1-item pattern has no deletions
        const uint32_t j = uint32_t(i) - b;
        const uint64_t rq = raw[q];
        const bool last = uint32_t(i) + 1 == e;
        const uint64_t incl = last ? rq : pre[i + 1];
        // tokens before j keep their place, tokens after it move down by one (x B^-1)
        uint64_t h = pre[i] + (rq - incl) * binv;
        if (start[i] && !last && !start[i + 1]) {
            const int32_t nx = items[i + 1];
            h += (pf_token(nx, 1) - pf_token(nx, 0)) * pf_pow(j);
        }
        const int32_t sq = sup[q];
        h = pf_final(h, len, sq, closed, hmask);
        uint64_t slot = h & tmask;
        for (uint32_t p; (p = table[slot]) != kPfEmpty; slot = (slot + 1) & tmask) {
            if (hash[p] != h) continue;
            const uint32_t pb = ioff[p];
            if (ioff[p + 1] - pb != len) continue;
            if (closed && sup[p] != sq) continue;
            if (drop[p]) continue;  // (already dropped by another deletion: set-only flag)
            if (pf_same(items, start, pb, b, j, len)) drop[p] = 1;
        }
    }
}

unsigned pf_grid(uint64_t work) {
    return unsigned(std::min<uint64_t>(std::max<uint64_t>((work + kPfBlock - 1) / kPfBlock, 1), kPfMaxGrid));
}

// FSM_PF_HASH_BITS=k (0..64): the mask of the hash bits in use (test hook, read once per call)
uint64_t pf_hash_mask() {
    const char* v = std::getenv("FSM_PF_HASH_BITS");
    if (!v || !*v) return ~0ull;
    char* end = nullptr;
    const long k = std::strtol(v, &end, 10);
    if (end == v || *end || k < 0 || k >= 64) return ~0ull;
    return (uint64_t(1) << k) - 1;
}

// result arrays as spade_mine allocates them (fsm_patterns_free hands them to big_give)
template <class T> T* pf_result_array(size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    T* p = bytes >= 4 * kHugeBlock ? static_cast<T*>(big_take((bytes + kHugeBlock - 1) & ~(kHugeBlock - 1)))
                                   : static_cast<T*>(std::malloc(bytes));
    if (!p) throw Error(FSM_ENOMEM, "malloc failed");
    return p;
}

struct ResultGuard {
    fsm_patterns* p = nullptr;
    ~ResultGuard() {
        if (!p) return;
        big_give(p->support);
        big_give(p->pat_off);
        big_give(p->set_off);
        big_give(p->items);
        std::free(p);
    }
};

// drop[] -> the kept patterns in input order (two passes over pattern slices: sizes, fill)
void pf_compact(const fsm_patterns* in, const uint8_t* drop, fsm_patterns* out, int64_t* kept_idx) {
    const int64_t n = in->n;
    const int64_t nthr = n >= 65536 ? host_threads() : 1;
    std::vector<int64_t> cp(size_t(nthr) + 1, 0), cs(size_t(nthr) + 1, 0), ci(size_t(nthr) + 1, 0);
    par_slices(nthr, n, [&](int64_t t, int64_t p0, int64_t p1) {
        int64_t a = 0, b = 0, c = 0;
        for (int64_t p = p0; p < p1; ++p) {
            if (drop[p]) continue;
            ++a;
            b += in->pat_off[p + 1] - in->pat_off[p];
            c += in->set_off[in->pat_off[p + 1]] - in->set_off[in->pat_off[p]];
        }
        cp[size_t(t) + 1] = a;
        cs[size_t(t) + 1] = b;
        ci[size_t(t) + 1] = c;
    });
    for (int64_t t = 0; t < nthr; ++t) {
        cp[size_t(t) + 1] += cp[size_t(t)];
        cs[size_t(t) + 1] += cs[size_t(t)];
        ci[size_t(t) + 1] += ci[size_t(t)];
    }
    const int64_t kn = cp[size_t(nthr)], ks = cs[size_t(nthr)], ki = ci[size_t(nthr)];
    out->support = pf_result_array<int32_t>(size_t(kn));
    out->pat_off = pf_result_array<int64_t>(size_t(kn) + 1);
    out->set_off = pf_result_array<int64_t>(size_t(ks) + 1);
    out->items = pf_result_array<int32_t>(size_t(ki));
    out->n = kn;
    out->n_sets = ks;
    out->n_items = ki;
    out->pat_off[kn] = ks;
    out->set_off[ks] = ki;
    par_slices(nthr, n, [&](int64_t t, int64_t p0, int64_t p1) {
        int64_t a = cp[size_t(t)], b = cs[size_t(t)], c = ci[size_t(t)];
        for (int64_t p = p0; p < p1; ++p) {
            if (drop[p]) continue;
            const int64_t s0 = in->pat_off[p], s1 = in->pat_off[p + 1];
            const int64_t i0 = in->set_off[s0], i1 = in->set_off[s1];
            out->support[a] = in->support[p];
            out->pat_off[a] = b;
            if (kept_idx) kept_idx[a] = p;
            ++a;
            for (int64_t s = s0; s < s1; ++s) out->set_off[b++] = c + (in->set_off[s] - i0);
            std::memcpy(out->items + c, in->items + i0, size_t(i1 - i0) * sizeof(int32_t));
            c += i1 - i0;
        }
    });
}

}  // namespace

// The CSR checks of fsm_patterns_filter and fsm_patterns_support (`who` names the caller in
// the messages; fsm_patterns_support takes a NULL support array), and the two compact arrays
// the kernels read instead of the 64-bit offsets: ioff[p] = first flat item of pattern p,
// start[i] = item i opens an itemset.  Split over the host threads by patterns.
void pf_validate(const fsm_patterns* in, const char* who, bool need_support, std::vector<uint32_t>& ioff,
                 std::vector<uint8_t>& start) {
    const std::string pre = std::string(who) + ": ";
    const int64_t n = in->n, ns = in->n_sets, ni = in->n_items;
    if ((need_support && !in->support) || !in->pat_off || !in->set_off || !in->items)
        throw Error(FSM_EINVAL, pre + "null pattern arrays");
    if (ns < n || ni < ns) throw Error(FSM_EINVAL, pre + "fewer itemsets than patterns or items than itemsets");
    if (in->pat_off[0] != 0 || in->pat_off[n] != ns)
        throw Error(FSM_EINVAL, pre + "pat_off must run from 0 to n_sets");
    if (in->set_off[0] != 0 || in->set_off[ns] != ni)
        throw Error(FSM_EINVAL, pre + "set_off must run from 0 to n_items");
    ioff.resize(size_t(n) + 1);
    start.resize(size_t(ni));
    const int64_t nthr = n >= 65536 ? host_threads() : 1;
    std::vector<int64_t> bad(size_t(nthr), -1);
    std::vector<const char*> why(size_t(nthr), nullptr);
    par_slices(nthr, n, [&](int64_t t, int64_t p0, int64_t p1) {
        auto fail = [&](int64_t p, const char* m) {
            bad[size_t(t)] = p;
            why[size_t(t)] = m;
        };
        for (int64_t p = p0; p < p1; ++p) {
            const int64_t s0 = in->pat_off[p], s1 = in->pat_off[p + 1];
            if (s0 < 0 || s1 > ns || s0 > s1) return fail(p, "pat_off is not monotone");
            if (s0 == s1) return fail(p, "a pattern without itemsets");
            if (in->set_off[s0] < 0 || in->set_off[s0] > ni) return fail(p, "set_off is not monotone");
            ioff[size_t(p)] = uint32_t(in->set_off[s0]);
            for (int64_t s = s0; s < s1; ++s) {
                const int64_t i0 = in->set_off[s], i1 = in->set_off[s + 1];
                if (i0 < 0 || i1 > ni || i0 > i1) return fail(p, "set_off is not monotone");
                if (i0 == i1) return fail(p, "an empty itemset");
                start[size_t(i0)] = 1;
                for (int64_t i = i0 + 1; i < i1; ++i) {
                    if (in->items[i - 1] >= in->items[i]) return fail(p, "items of an itemset are not strictly ascending");
                    start[size_t(i)] = 0;
                }
            }
        }
    });
    for (int64_t t = 0; t < nthr; ++t)
        if (bad[size_t(t)] >= 0)
            throw Error(FSM_EINVAL, pre + why[size_t(t)] + " (pattern " + std::to_string(bad[size_t(t)]) + ")");
    ioff[size_t(n)] = uint32_t(ni);
}

void patterns_filter(fsm_ctx* ctx, const fsm_patterns* in, int32_t keep, fsm_patterns** out, int64_t* kept_idx) {
    const int64_t n = in->n, ni = in->n_items;
    if (n < 0 || in->n_sets < 0 || ni < 0) throw Error(FSM_EINVAL, "fsm_patterns_filter: negative sizes");
    constexpr int64_t kLimit = (int64_t(1) << 32) - 2;
    if (n >= kLimit || ni >= kLimit)
        throw Error(FSM_ELIMIT, "fsm_patterns_filter: 2^32 - 2 or more patterns or items");
    ResultGuard res;
    res.p = static_cast<fsm_patterns*>(std::calloc(1, sizeof(fsm_patterns)));
    if (!res.p) throw Error(FSM_ENOMEM, "calloc failed");
    res.p->total = in->total;
    res.p->minsup = in->minsup;
    if (n == 0) {
        if (in->n_sets != 0 || ni != 0) throw Error(FSM_EINVAL, "fsm_patterns_filter: itemsets or items without patterns");
        fsm_patterns empty{};
        const int64_t zero = 0;
        empty.pat_off = empty.set_off = const_cast<int64_t*>(&zero);
        pf_compact(&empty, nullptr, res.p, kept_idx);
        ctx->kstats.clear();
        *out = res.p;
        res.p = nullptr;
        return;
    }
    std::vector<uint32_t> ioff;
    std::vector<uint8_t> start, drop;
    pf_validate(in, "fsm_patterns_filter", true, ioff, start);

    const int closed = keep == FSM_KEEP_CLOSED;
    const uint64_t hmask = pf_hash_mask();
    uint64_t binv = kPfB;  // Newton: x <- x (2 - B x) doubles the correct low bits (3 to 96)
    for (int k = 0; k < 5; ++k) binv *= 2 - kPfB * binv;
    uint64_t slots = 16;
    while (slots < 2 * uint64_t(n)) slots <<= 1;
    const uint64_t tmask = slots - 1;

    // the input is valid: device work from here on
    FSM_HIP(hipSetDevice(ctx->opts.device));
    hipStream_t s = ctx->stream;
    // (an error below must not free the host arrays under a copy still queued on the stream)
    struct SyncOnExit {
        hipStream_t s;
        ~SyncOnExit() { (void)hipStreamSynchronize(s); }
    } sync_on_exit{s};
    KernelClock clock(s);
    const size_t un = size_t(n), ui = size_t(ni);
    DevBuf d_items(ui * 4), d_start(ui), d_ioff((un + 1) * 4), d_sup(un * 4);
    DevBuf d_pre(ui * 8), d_pid(ui * 4), d_raw(un * 8), d_hash(un * 8);
    DevBuf d_table(size_t(slots) * 4), d_drop(un);
    FSM_HIP(hipMemcpyAsync(d_items.p, in->items, ui * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_start.p, start.data(), ui, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_ioff.p, ioff.data(), (un + 1) * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemcpyAsync(d_sup.p, in->support, un * 4, hipMemcpyHostToDevice, s));
    FSM_HIP(hipMemsetAsync(d_table.p, 0xFF, size_t(slots) * 4, s));
    FSM_HIP(hipMemsetAsync(d_drop.p, 0, un, s));

    size_t tk = clock.begin("k_pf_hash");
    hipLaunchKernelGGL(k_pf_hash, dim3(pf_grid(uint64_t(n))), dim3(kPfBlock), 0, s, d_items.as<int32_t>(),
                       d_start.as<uint8_t>(), d_ioff.as<uint32_t>(), d_sup.as<int32_t>(), uint32_t(n), closed, hmask,
                       d_pre.as<uint64_t>(), d_pid.as<uint32_t>(), d_raw.as<uint64_t>(), d_hash.as<uint64_t>());
    FSM_LAUNCHED("k_pf_hash", s);
    // items + start read, prefix + owner written per item; offsets + support read, two hashes written per pattern
    clock.end(tk, ni * (4 + 1 + 8 + 4) + n * (4 + 4 + 8 + 8));

    tk = clock.begin("k_pf_insert");
    hipLaunchKernelGGL(k_pf_insert, dim3(pf_grid(uint64_t(n))), dim3(kPfBlock), 0, s, d_hash.as<uint64_t>(),
                       uint32_t(n), d_table.as<uint32_t>(), tmask);
    FSM_LAUNCHED("k_pf_insert", s);
    clock.end(tk, n * (8 + 4));  // hash read, one slot claimed

    tk = clock.begin("k_pf_probe");
    hipLaunchKernelGGL(k_pf_probe, dim3(pf_grid(uint64_t(ni))), dim3(kPfBlock), 0, s, d_items.as<int32_t>(),
                       d_start.as<uint8_t>(), d_ioff.as<uint32_t>(), d_sup.as<int32_t>(), d_pre.as<uint64_t>(),
                       d_pid.as<uint32_t>(), d_raw.as<uint64_t>(), d_hash.as<uint64_t>(), d_table.as<uint32_t>(),
                       tmask, uint64_t(ni), closed, hmask, binv, d_drop.as<uint8_t>());
    FSM_LAUNCHED("k_pf_probe", s);
    // per deletion: owner, prefix hash, item, start flag, one table slot; per pattern: its hashes,
    // offset and support once, its drop flag
    clock.end(tk, ni * (4 + 8 + 4 + 1 + 4) + n * (8 + 8 + 4 + 4 + 1));

    drop.resize(un);
    FSM_HIP(hipMemcpyAsync(drop.data(), d_drop.p, un, hipMemcpyDeviceToHost, s));
    clock.finish(ctx->kstats);  // synchronizes the stream
    pf_compact(in, drop.data(), res.p, kept_idx);
    *out = res.p;
    res.p = nullptr;
}

}  // namespace fsm
