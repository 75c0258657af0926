// Filtered sampling on gfx950: repetition / presence penalties, top-k, top-p, then the keyed categorical draw of random.hip
// restricted to the kept set.
//   reference: funasr-qwen4b-mlx/src/model.rs:1333-1383 (sample_top_k_p: presence penalty, * (1/T), topk_axis -> threshold ->
//              where(x >= thr, x, -inf) -> categorical), step-audio2-mlx/src/llm.rs:440-474 (apply_repetition_penalty:
//              x > 0 ? x / r : x * r), gpt-sovits-mlx/src/sampling.rs:122-215 (repetition penalty, top-p, temperature, top-k).
// The rule, one IEEE float32 operation per element and step (include/omx.h, omx_sample_filtered):
//   x = f32(logit);  seen: x = x > 0 ? x / r : x * r, then x = x - q;  y = x * (1/T);
//   top-k: keep y >= (k-th largest y), ties at the threshold all kept (the reference's `ge`);
//   top-p on the survivors: with Z = sum exp(y - max) over them, keep v iff the mass of survivors STRICTLY greater than y_v is
//          < top_p * Z -- "the smallest set reaching p" made independent of the sort order: a tie group stays or goes whole and the
//          maximum always stays.  This differs on purpose from gpt-sovits-mlx/src/sampling.rs:180-203, which drops a token when the
//          INCLUSIVE mass exceeds p (and so can drop every token, and depends on the order of equal values);
//   token = argmax over the kept set of y + gumbel(word v of a V-word draw), first index on ties.
// Structure: a radix select on the order-preserving u32 image of y, most significant digit first; per digit a COUNT histogram serves
// top-k and a MASS histogram (sum of exp(y - max)) serves top-p, the same descent for both.  The row was just written by the lm_head
// launch and is L2 resident; a level re-reads it.  Two forms: one block per row with 8-bit digits (short rows, many rows: one launch),
// and a launch per level over many blocks with 11 + 11 + 10-bit digits (the engine's step and vocabulary-sized single rows; DESIGN 4.5,
// EXPERIMENTS R8-1 for why).  Masses are accumulated as 2^-40 fixed point in 64-bit integers: exact, order independent sums (the draw
// replays bit for bit), no chain of float roundings; the only float error is expf's.  Gumbel noise (a Threefry block and two double
// logs per entry) is computed only for kept entries, after the threshold is known.
#include "sample_filter.hpp"
#include "random.hpp"
#include "vec.hpp"
#include "workspace.hpp"
#include <stddef.h>

namespace omx {

namespace {

constexpr int kSelThreads = 1024;
constexpr int kCopies = 16;
constexpr float kMassOne = 1099511627776.0f;   // 2^40

// order-preserving image of y: a > b <=> key(a) > key(b); -0 and +0 share a key (they compare equal); NaN = 0, below everything
__device__ __forceinline__ uint32_t y_key(float y) {
    uint32_t u = __float_as_uint(y);
    if (y == 0.f) u = 0u;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return y != y ? 0u : u;
}
__device__ __forceinline__ float key_y(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ __forceinline__ float apply_rule(float x, bool is_seen, const RowRule& r) {
    if (is_seen) {
        if (r.rep != 1.f) x = x > 0.f ? x / r.rep : x * r.rep;
        if (r.pres != 0.f) x = x - r.pres;
    }
    return x * r.inv_temp;
}

// f(v, y) for every v of the row handled by this thread of a group of `nthr` threads (`tid` among them); 16-bit rows are read eight
// elements per load once the address is 16-byte aligned
template <int DT, class F>
__device__ __forceinline__ void for_each_y(const typename Elem<DT>::T* __restrict__ row, const uint8_t* __restrict__ seen, int V,
                                           const RowRule& r, int tid, int nthr, F f) {
    if (sizeof(typename Elem<DT>::T) == 2) {
        int head = (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 1);
        head = head < V ? head : V;
        const int chunks = (V - head) >> 3;
        if (tid < head) f(tid, apply_rule(Elem<DT>::ld(row + tid), seen && seen[tid], r));
        const u32x4* body = reinterpret_cast<const u32x4*>(row + head);
        for (int c = tid; c < chunks; c += nthr) {
            const u32x4 w = body[c];
            const int v0 = head + (c << 3);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint16_t h = (uint16_t)(w[j >> 1] >> ((j & 1) * 16));
                const float x = DT == OMX_BFLOAT16 ? bf16_to_f32(h) : (float)__builtin_bit_cast(f16_t, h);
                f(v0 + j, apply_rule(x, seen && seen[v0 + j], r));
            }
        }
        const int tail = head + (chunks << 3);
        if (tail + tid < V) f(tail + tid, apply_rule(Elem<DT>::ld(row + tail + tid), seen && seen[tail + tid], r));   // < 8 entries
    } else {
        for (int v = tid; v < V; v += nthr) f(v, apply_rule(Elem<DT>::ld(row + v), seen && seen[v], r));
    }
}

// one-block form: histograms live in LDS in 16 copies (one per lane mod 16) -- logits crowd a few exponents, so most of a wave hits
// the same bin and one copy would serialise it
struct SelectLds {
    uint32_t cnt[256 * kCopies];
    unsigned long long mass[256 * kCopies];
    uint32_t rc[256], rc0[256], gc[16];            // per-bin counts of the current pass / of the first (whole-row) pass; sums of 16 bins
    unsigned long long rm[256], rm0[256], gm[16];
    float red[kSelThreads / 64];
    uint32_t bin;
    uint32_t above_cnt, kept;
    unsigned long long above_mass, z;
};

// one histogram pass over the entries whose key starts with `prefix` (level = digits already fixed); rc / rm = per-bin totals
template <int DT>
__device__ void hist_pass(SelectLds& L, const typename Elem<DT>::T* row, const uint8_t* seen, int V, const RowRule& r, uint32_t prefix,
                          int level, bool want_mass, float ymax) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 256 * kCopies; i += kSelThreads) {
        L.cnt[i] = 0;
        L.mass[i] = 0;
    }
    __syncthreads();
    const int shift = 24 - 8 * level, copy = tid & (kCopies - 1);
    for_each_y<DT>(row, seen, V, r, tid, kSelThreads, [&](int, float y) {
        const uint32_t key = y_key(y);
        if (level == 0 || (key >> (shift + 8)) == prefix) {
            const int slot = (int)((key >> shift) & 255u) * kCopies + copy;
            atomicAdd(&L.cnt[slot], 1u);
            if (want_mass) {
                float e = expf(y - ymax);
                e = e == e ? e : 0.f;   // NaN entries, inf - inf
                atomicAdd(&L.mass[slot], (unsigned long long)(e * kMassOne));
            }
        }
    });
    __syncthreads();
    if (tid < 256) {
        uint32_t c = 0;
        unsigned long long m = 0;
#pragma unroll
        for (int j = 0; j < kCopies; ++j) {
            const int jj = (j + tid) & (kCopies - 1);
            c += L.cnt[tid * kCopies + jj];
            m += L.mass[tid * kCopies + jj];
        }
        L.rc[tid] = c;
        L.rm[tid] = m;
    }
    __syncthreads();
}

// count and mass of the bins ABOVE bin b of one level (threads 0..255, bin = threadIdx.x); all threads call
__device__ void above_bins(SelectLds& L, const uint32_t* rc, const unsigned long long* rm, uint32_t& c_out, unsigned long long& m_out) {
    const int tid = threadIdx.x;
    if (tid < 16) {
        uint32_t c = 0;
        unsigned long long m = 0;
        for (int j = 0; j < 16; ++j) {
            c += rc[tid * 16 + j];
            m += rm[tid * 16 + j];
        }
        L.gc[tid] = c;
        L.gm[tid] = m;
    }
    __syncthreads();
    uint32_t c = 0;
    unsigned long long m = 0;
    if (tid < 256) {
        for (int g = (tid >> 4) + 1; g < 16; ++g) {
            c += L.gc[g];
            m += L.gm[g];
        }
        for (int b = tid + 1; b < ((tid >> 4) + 1) * 16; ++b) {
            c += rc[b];
            m += rm[b];
        }
    }
    c_out = c;
    m_out = m;
}

// The selection of one row by one block of kSelThreads threads.  Returns (to every thread) the key image of the final threshold
// on y and the number of entries at or above it.  top_k <= 0 or >= V: off; top_p >= 1: off.
template <int DT>
__device__ void row_select(SelectLds& L, const typename Elem<DT>::T* row, const uint8_t* seen, int V, const RowRule& r, int top_k,
                           float top_p, uint32_t& thr_out, uint32_t& kept_out) {
    const int tid = threadIdx.x;
    const bool k_on = top_k > 0 && top_k < V, p_on = top_p < 1.f;
    uint32_t thr = 0, kept = (uint32_t)V;
    if (!k_on && !p_on) {
        thr_out = thr;
        kept_out = kept;
        return;
    }
    float ymax = 0.f;
    if (p_on) {   // the masses are exp(y - max)
        float mx = -INFINITY;
        for_each_y<DT>(row, seen, V, r, tid, kSelThreads, [&](int, float y) { mx = fmaxf(mx, y); });
        mx = wave_max(mx);
        if ((tid & 63) == 0) L.red[tid >> 6] = mx;
        __syncthreads();
        for (int w = 0; w < kSelThreads / 64; ++w) mx = fmaxf(mx, L.red[w]);
        ymax = mx;
    }
    unsigned long long z = 0;
    bool have_rc0 = false;
    if (k_on) {   // the k-th largest key, digit by digit; the masses met on the way sum to Z of the survivors
        uint32_t prefix = 0;
        if (tid == 0) {
            L.above_cnt = 0;
            L.above_mass = 0;
        }
        for (int level = 0; level < 4; ++level) {
            hist_pass<DT>(L, row, seen, V, r, prefix, level, p_on, ymax);
            if (level == 0 && p_on && tid < 256) {
                L.rc0[tid] = L.rc[tid];
                L.rm0[tid] = L.rm[tid];
            }
            uint32_t ac;
            unsigned long long am;
            above_bins(L, L.rc, L.rm, ac, am);
            const uint32_t a_cnt = L.above_cnt;
            const unsigned long long a_mass = L.above_mass;
            __syncthreads();
            if (tid < 256 && a_cnt + ac < (uint32_t)top_k && (uint32_t)top_k <= a_cnt + ac + L.rc[tid]) {   // exactly one bin
                L.bin = (uint32_t)tid;
                L.above_cnt = a_cnt + ac;
                L.above_mass = a_mass + am;
                L.kept = a_cnt + ac + L.rc[tid];
                L.z = a_mass + am + L.rm[tid];
            }
            __syncthreads();
            prefix = (prefix << 8) | L.bin;
        }
        thr = prefix;
        kept = L.kept;
        z = L.z;
        have_rc0 = p_on;
        __syncthreads();
    }
    if (p_on) {   // the lowest key whose strictly-greater mass is < p * Z, digit by digit; then the higher of the two thresholds
        uint32_t prefix = 0;
        if (tid == 0) {
            L.above_cnt = 0;
            L.above_mass = 0;
        }
        double pz = 0.0;
        for (int level = 0; level < 4; ++level) {
            const uint32_t* rc = L.rc;
            const unsigned long long* rm = L.rm;
            if (level == 0 && have_rc0) {
                rc = L.rc0;
                rm = L.rm0;
            } else {
                hist_pass<DT>(L, row, seen, V, r, prefix, level, true, ymax);
            }
            uint32_t ac;
            unsigned long long am;
            above_bins(L, rc, rm, ac, am);
            if (tid == 0) L.bin = 256u;
            __syncthreads();
            if (level == 0 && !k_on) {   // no top-k: every entry survives, Z = the whole row
                unsigned long long t = 0;
                for (int g = 0; g < 16; ++g) t += L.gm[g];
                z = t;
            }
            if (level == 0) pz = (double)top_p * (double)z;
            const uint32_t a_cnt = L.above_cnt;
            const unsigned long long a_mass = L.above_mass;
            if (tid < 256 && rc[tid] > 0 && (double)(a_mass + am) < pz) atomicMin(&L.bin, (uint32_t)tid);
            __syncthreads();
            const uint32_t b = L.bin;
            __syncthreads();
            if (b == 256u) break;   // (uniform; level 0 only) a row without finite mass, Z = 0 or NaN: top-p has nothing to compare
            if (tid == (int)b) {
                L.above_cnt = a_cnt + ac;
                L.above_mass = a_mass + am;
                L.kept = a_cnt + ac + rc[tid];
            }
            __syncthreads();
            prefix = (prefix << 8) | b;
            if (level == 3) {
                if (prefix > thr) {
                    thr = prefix;
                    kept = L.kept;
                }
            }
        }
        __syncthreads();
    }
    thr_out = thr;
    kept_out = kept;
}

// out[r] = the draw of row r under the rule; one block per row selects and draws (noise only for kept entries)
template <int DT>
__global__ __launch_bounds__(kSelThreads) void sample_filtered_kernel(uint32_t* __restrict__ out, const typename Elem<DT>::T* __restrict__ logits,
                                                                      const uint8_t* __restrict__ seen, const uint32_t* __restrict__ key,
                                                                      int V, uint64_t n_words, RowRule rule, int top_k, float top_p,
                                                                      int greedy, float* __restrict__ thr_f, int32_t* __restrict__ kept_i) {
    __shared__ SelectLds L;
    __shared__ unsigned long long red[kSelThreads / 64];
    const uint64_t r = blockIdx.x;
    const typename Elem<DT>::T* row = logits + r * (uint64_t)V;
    uint32_t thr, kept;
    row_select<DT>(L, row, seen, V, rule, greedy ? 0 : top_k, greedy ? 1.f : top_p, thr, kept);
    const uint32_t k0 = greedy ? 0u : key[0], k1 = greedy ? 0u : key[1];
    unsigned long long best = 0;
    for_each_y<DT>(row, seen, V, rule, threadIdx.x, kSelThreads, [&](int v, float y) {
        if (y_key(y) >= thr) {
            const float g = greedy ? 0.f : gumbel_from_word(random_word(k0, k1, r * (uint64_t)V + (uint64_t)v, n_words));
            const unsigned long long kx = sample_key(greedy ? y : y + g, (uint32_t)v);
            best = kx > best ? kx : best;
        }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kSelThreads / 64; ++w) best = red[w] > best ? red[w] : best;
        out[r] = ~(uint32_t)(best & 0xFFFFFFFFull);
        if (thr_f) thr_f[r] = thr ? key_y(thr) : -INFINITY;
        if (kept_i) kept_i[r] = (int32_t)kept;
    }
}

// ---- the selection as a few launches over many blocks (the engine's step, and one-row calls at vocabulary sizes) ----
// One block re-reading a 300 KB row is latency bound (a wave has one 16-byte load in flight) and funnels 150 000 LDS atomics through
// one CU.  Here a level of the descent is one launch of kHistBlocks blocks: each block histograms its share of the row in LDS and adds
// its non-empty bins to the level's histogram in the workspace; the NEXT launch's blocks each scan that histogram (2 048 bins, eight
// per thread) and so all know the digit chosen -- the kernel boundary is the only cross-block hand-off.  Digits are 11 + 11 + 10 bits.
// Slots: 0 = the whole row (first level of both descents), 1 / 2 = top-k's second / third level, 3 / 4 = top-p's.
constexpr int kBins = 2048, kSlots = 5, kHistThreads = 256, kHistBlocks = 64, kOpPartials = 128;
constexpr int kMultiLaunchMin = 16384;   // shorter rows: the one-block kernel (launch count beats pass time there)
struct SelCarry {   // the descent after a level: digits so far, what lies above them; at the end: threshold key, kept count, Z
    uint32_t prefix, above_cnt, kept, none;
    unsigned long long above_mass, z;
};
struct SelWs {
    uint32_t maxkey, thr, kept, pad;
    SelCarry carry[kSlots + 1];
    uint32_t cnt[kSlots][kBins];
    unsigned long long mass[kSlots][kBins];
    unsigned long long partials[kOpPartials];   // omx_sample_filtered's own noise partials
};
struct ScanLds {
    uint32_t tc[256], gc[16], bin;
    unsigned long long tm[256], gm[16];
    SelCarry out;
};
__device__ __forceinline__ int level_bits(int level) { return level == 2 ? 10 : 11; }

// this thread's eight bins of a level's histogram, and the count / mass of every bin above them (256 threads, all call)
__device__ __forceinline__ void scan_level(ScanLds& S, const uint32_t* __restrict__ gcnt, const unsigned long long* __restrict__ gmass, int nbins,
                           uint32_t (&c)[8], unsigned long long (&m)[8], uint32_t& ac, unsigned long long& am) {
    const int tid = threadIdx.x;
    uint32_t tc = 0;
    unsigned long long tm = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = tid * 8 + j;
        c[j] = b < nbins ? gcnt[b] : 0u;
        m[j] = b < nbins ? gmass[b] : 0ull;
        tc += c[j];
        tm += m[j];
    }
    __syncthreads();   // (S is reused from an earlier scan)
    S.tc[tid] = tc;
    S.tm[tid] = tm;
    if (tid == 0) S.bin = (uint32_t)kBins;
    __syncthreads();
    if (tid < 16) {
        uint32_t gc = 0;
        unsigned long long gm = 0;
        for (int j = 0; j < 16; ++j) {
            gc += S.tc[tid * 16 + j];
            gm += S.tm[tid * 16 + j];
        }
        S.gc[tid] = gc;
        S.gm[tid] = gm;
    }
    __syncthreads();
    ac = 0;
    am = 0;
    for (int g = (tid >> 4) + 1; g < 16; ++g) {
        ac += S.gc[g];
        am += S.gm[g];
    }
    for (int t = tid + 1; t < ((tid >> 4) + 1) * 16; ++t) {
        ac += S.tc[t];
        am += S.tm[t];
    }
}

// one level of top-k's descent: the bin holding the k-th largest.  Returns the carry after it (to every thread).
__device__ __forceinline__ SelCarry decide_k(ScanLds& S, const SelWs* ws, int slot, int level, const SelCarry& in, uint32_t top_k) {
    uint32_t c[8], ac;
    unsigned long long m[8], am;
    scan_level(S, ws->cnt[slot], ws->mass[slot], 1 << level_bits(level), c, m, ac, am);
    uint32_t run = in.above_cnt + ac;
    unsigned long long runm = in.above_mass + am;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
        if (run < top_k && top_k <= run + c[j]) {   // exactly one bin of one thread
            SelCarry o;
            o.prefix = (in.prefix << level_bits(level)) | (uint32_t)(threadIdx.x * 8 + j);
            o.above_cnt = run;
            o.above_mass = runm;
            o.kept = run + c[j];
            o.z = runm + m[j];
            o.none = 0;
            S.out = o;
        }
        run += c[j];
        runm += m[j];
    }
    __syncthreads();
    return S.out;
}

// one level of top-p's descent: the lowest non-empty bin whose strictly-greater mass is < pz
__device__ __forceinline__ SelCarry decide_p(ScanLds& S, const SelWs* ws, int slot, int level, const SelCarry& in, double pz, bool whole_row, unsigned long long& total) {
    uint32_t c[8], ac;
    unsigned long long m[8], am;
    scan_level(S, ws->cnt[slot], ws->mass[slot], 1 << level_bits(level), c, m, ac, am);
    if (whole_row) {   // Z of the whole row (no top-k): pz follows from it
        unsigned long long t = 0;
        for (int g = 0; g < 16; ++g) t += S.gm[g];
        total = t;
        pz = pz * (double)t;
    }
    uint32_t run = in.above_cnt + ac;
    unsigned long long runm = in.above_mass + am;
    uint32_t rc[8];
    unsigned long long rm[8];
#pragma unroll
    for (int j = 7; j >= 0; --j) {
        rc[j] = run;
        rm[j] = runm;
        if (c[j] > 0 && (double)runm < pz) atomicMin(&S.bin, (uint32_t)(threadIdx.x * 8 + j));
        run += c[j];
        runm += m[j];
    }
    __syncthreads();
    const uint32_t b = S.bin;
    if (b == (uint32_t)kBins) {   // a row without finite mass (Z = 0 or NaN): top-p has nothing to compare
        SelCarry o = in;
        o.none = 1;
        return o;
    }
    if ((b >> 3) == threadIdx.x) {
        SelCarry o;
        const int j = (int)(b & 7u);
        uint32_t rcj = 0, cj = 0;   // (picked by a chain of selects: an index known only at run time would put the arrays in scratch)
        unsigned long long rmj = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            rcj = i == j ? rc[i] : rcj;
            rmj = i == j ? rm[i] : rmj;
            cj = i == j ? c[i] : cj;
        }
        o.prefix = (in.prefix << level_bits(level)) | b;
        o.above_cnt = rcj;
        o.above_mass = rmj;
        o.kept = rcj + cj;
        o.z = in.z;
        o.none = in.none;
        S.out = o;
    }
    __syncthreads();
    return S.out;
}

// the descent up to the state the launch of `slot` needs (slot == kSlots: to the end -> out.prefix = threshold key, out.kept);
// block 0 leaves what it derived in ws->carry for the later launches
__device__ __forceinline__ SelCarry resolve(ScanLds& S, SelWs* ws, int slot, uint32_t top_k, float top_p, int V, bool k_on, bool p_on) {
    const SelCarry zero = {0u, 0u, 0u, 0u, 0ull, 0ull};
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    SelCarry o = zero;
    unsigned long long unused = 0;
    if (slot == 1) {
        o = decide_k(S, ws, 0, 0, zero, top_k);
        if (lead) ws->carry[1] = o;
    } else if (slot == 2) {
        o = decide_k(S, ws, 1, 1, ws->carry[1], top_k);
        if (lead) ws->carry[2] = o;
    } else if (slot == 3) {   // top-k's end (threshold, kept, Z of the survivors), then top-p's first level on the whole-row histogram
        SelCarry kend = zero;
        kend.kept = (uint32_t)V;
        double pz = (double)top_p;
        unsigned long long total = 0;
        if (k_on) {
            kend = decide_k(S, ws, 2, 2, ws->carry[2], top_k);
            pz = pz * (double)kend.z;
        }
        o = decide_p(S, ws, 0, 0, zero, pz, !k_on, total);
        if (!k_on) kend.z = total;
        o.z = kend.z;
        if (lead) {
            ws->carry[3] = kend;
            ws->carry[4] = o;
        }
    } else if (slot == 4) {
        const SelCarry in = ws->carry[4];
        o = decide_p(S, ws, 3, 1, in, (double)top_p * (double)in.z, false, unused);
        if (lead) ws->carry[5] = o;
    } else if (slot == kSlots) {
        if (p_on) {
            const SelCarry in = ws->carry[5], kend = ws->carry[3];
            o = decide_p(S, ws, 4, 2, in, (double)top_p * (double)in.z, false, unused);
            if (o.none || o.prefix <= kend.prefix) {   // the higher of the two thresholds
                o.prefix = kend.prefix;
                o.kept = kend.kept;
            }
        } else if (k_on) {
            o = decide_k(S, ws, 2, 2, ws->carry[2], top_k);
        } else {
            o.kept = (uint32_t)V;
        }
    }
    return o;
}

// The bodies of the launches, written once: the one-row kernels below call them as they are, the row-batched ones of a batch step
// (grid.y = the row) with the row's own arguments.  Blocks and threads are counted along x.
template <int DT>
__device__ __forceinline__ void select_max_body(SelWs* __restrict__ ws, const typename Elem<DT>::T* __restrict__ row,
                                                const uint8_t* __restrict__ seen, int V, const RowRule& rule) {
    __shared__ uint32_t red[kHistThreads / 64];
    uint32_t best = 0;
    for_each_y<DT>(row, seen, V, rule, blockIdx.x * kHistThreads + threadIdx.x, gridDim.x * kHistThreads, [&](int, float y) {
        const uint32_t k = y_key(y);
        best = k > best ? k : best;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kHistThreads / 64; ++w) best = red[w] > best ? red[w] : best;
        atomicMax(&ws->maxkey, best);
    }
}
template <int DT>
__global__ __launch_bounds__(kHistThreads) void select_max_kernel(SelWs* __restrict__ ws, const typename Elem<DT>::T* __restrict__ row,
                                                                  const uint8_t* __restrict__ seen, int V, RowRule rule) {
    select_max_body<DT>(ws, row, seen, V, rule);
}

template <int DT>
__device__ __forceinline__ void select_hist_body(SelWs* __restrict__ ws, const typename Elem<DT>::T* __restrict__ row,
                                                 const uint8_t* __restrict__ seen, int V, const RowRule& rule, int slot, uint32_t top_k,
                                                 float top_p, int k_on, int p_on) {
    __shared__ ScanLds S;
    __shared__ uint32_t cnt[kBins];
    __shared__ unsigned long long mass[kBins];
    const int tid = threadIdx.x;
    const int level = slot == 0 ? 0 : (slot == 1 || slot == 3) ? 1 : 2;
    for (int i = tid; i < kBins; i += kHistThreads) {
        cnt[i] = 0;
        mass[i] = 0;
    }
    const SelCarry st = resolve(S, ws, slot, top_k, top_p, V, k_on, p_on);   // (ends in a barrier for slot > 0)
    __syncthreads();
    if (st.none) return;   // (uniform) top-p without finite mass: nothing further to count
    const uint32_t prefix = st.prefix;
    const float ymax = key_y(ws->maxkey);
    const int shift = level == 0 ? 21 : level == 1 ? 10 : 0, mshift = level == 1 ? 21 : 10;
    const uint32_t bmask = level == 2 ? 1023u : 2047u;
    for_each_y<DT>(row, seen, V, rule, blockIdx.x * kHistThreads + tid, gridDim.x * kHistThreads, [&](int, float y) {
        const uint32_t key = y_key(y);
        if (level == 0 || (key >> mshift) == prefix) {
            const uint32_t b = (key >> shift) & bmask;
            atomicAdd(&cnt[b], 1u);
            if (p_on) {
                float e = expf(y - ymax);
                e = e == e ? e : 0.f;   // NaN entries, inf - inf
                atomicAdd(&mass[b], (unsigned long long)(e * kMassOne));
            }
        }
    });
    __syncthreads();
    for (int i = tid; i < kBins; i += kHistThreads) {
        if (cnt[i]) {
            atomicAdd(&ws->cnt[slot][i], cnt[i]);
            if (p_on) atomicAdd(&ws->mass[slot][i], mass[i]);
        }
    }
}
template <int DT>
__global__ __launch_bounds__(kHistThreads) void select_hist_kernel(SelWs* __restrict__ ws, const typename Elem<DT>::T* __restrict__ row,
                                                                   const uint8_t* __restrict__ seen, int V, RowRule rule, int slot,
                                                                   uint32_t top_k, float top_p, int k_on, int p_on) {
    select_hist_body<DT>(ws, row, seen, V, rule, slot, top_k, top_p, k_on, p_on);
}

// [resolve], one block: the last level's decision -> ws->thr (key image of the final threshold), ws->kept; then (zero != 0) the
// histograms are cleared for the next selection -- a memset node costs a launch of its own (7.6 us traced)
__device__ __forceinline__ void select_resolve_body(SelWs* __restrict__ ws, uint32_t top_k, float top_p, int V, int k_on, int p_on, int zero) {
    __shared__ ScanLds S;
    const SelCarry end = resolve(S, ws, kSlots, top_k, top_p, V, k_on, p_on);
    __syncthreads();
    if (zero) {
        u32x4* h = reinterpret_cast<u32x4*>(&ws->cnt[0][0]);
        constexpr int n16 = (int)((sizeof(SelWs::cnt) + sizeof(SelWs::mass)) / 16);
        static_assert(offsetof(SelWs, cnt) % 16 == 0 && offsetof(SelWs, mass) == offsetof(SelWs, cnt) + sizeof(SelWs::cnt), "cnt | mass contiguous");
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int i = threadIdx.x; i < n16; i += kHistThreads) h[i] = z;
    }
    if (threadIdx.x == 0) {
        ws->maxkey = 0;
        ws->thr = end.prefix;
        ws->kept = end.kept;
    }
}
__global__ __launch_bounds__(kHistThreads) void select_resolve_kernel(SelWs* __restrict__ ws, uint32_t top_k, float top_p, int V, int k_on,
                                                                      int p_on, int zero) {
    select_resolve_body(ws, top_k, top_p, V, k_on, p_on, zero);
}

// [noise]: sample_noise_kernel (random.hip) restricted to the kept set {key(y) >= ws->thr}, penalties applied (ws == nullptr: nothing
// filtered).  n_words: the size of the draw the row's words belong to.
template <int DT>
__device__ __forceinline__ void filtered_noise_body(unsigned long long* __restrict__ partials, const typename Elem<DT>::T* __restrict__ logits,
                                                    const uint8_t* __restrict__ seen, uint32_t thr, uint32_t k0, uint32_t k1, int V,
                                                    uint64_t n_words, const RowRule& rule, int greedy) {
    __shared__ unsigned long long red[4];
    unsigned long long best = 0;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256) {
        const float y = apply_rule(Elem<DT>::ld(logits + v), seen && seen[v], rule);
        if (y_key(y) >= thr) {
            const float g = greedy ? 0.f : gumbel_from_word(random_word(k0, k1, (uint64_t)v, n_words));
            const unsigned long long kx = sample_key(greedy ? y : y + g, (uint32_t)v);
            best = kx > best ? kx : best;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = red[w] > best ? red[w] : best;
        partials[blockIdx.x] = best;
    }
}
template <int DT>
__global__ __launch_bounds__(256) void sample_filtered_noise_kernel(unsigned long long* __restrict__ partials,
                                                                    const typename Elem<DT>::T* __restrict__ logits,
                                                                    const uint8_t* __restrict__ seen, const SelWs* __restrict__ ws,
                                                                    const uint32_t* __restrict__ sub_key, int V, uint64_t n_words,
                                                                    RowRule rule, int greedy) {
    filtered_noise_body<DT>(partials, logits, seen, ws ? ws->thr : 0u, greedy ? 0u : sub_key[0], greedy ? 0u : sub_key[1], V, n_words, rule,
                            greedy);
}

// omx_sample_filtered's last launch on this path: the partials' maximum, the threshold and the kept count
__global__ __launch_bounds__(kOpPartials) void select_finish_kernel(uint32_t* out, float* thr_f, int32_t* kept_i, const SelWs* ws) {
    __shared__ unsigned long long red[kOpPartials / 64];
    unsigned long long best = ws->partials[threadIdx.x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kOpPartials / 64; ++w) best = red[w] > best ? red[w] : best;
        out[0] = ~(uint32_t)(best & 0xFFFFFFFFull);
        if (thr_f) thr_f[0] = ws->thr ? key_y(ws->thr) : -INFINITY;
        if (kept_i) kept_i[0] = (int32_t)ws->kept;
    }
}


__global__ void mark_seen_kernel(uint8_t* seen, int V, const StepState* st) {
    const uint32_t tok = st->cur_token;
    if (tok < (uint32_t)V) seen[tok] = 1;
}

// out[r, :] = the k largest values of x[r, :], ascending.  The select gives the k-th largest; the entries strictly above it (< k of
// them) are gathered and rank-sorted in LDS, the rest of the k slots are copies of the threshold value.
constexpr int kTopkMax = 4096;
static_assert(kTopkMax * sizeof(uint32_t) <= sizeof(SelectLds::mass), "the gathered keys reuse the mass histogram");
template <int DT>
__global__ __launch_bounds__(kSelThreads) void topk_values_kernel(typename Elem<DT>::T* __restrict__ out,
                                                                  const typename Elem<DT>::T* __restrict__ x, int V, int k) {
    __shared__ SelectLds L;
    __shared__ uint32_t n_above;
    uint32_t* keys = reinterpret_cast<uint32_t*>(L.mass);   // free once the select is done: kTopkMax keys fit
    const uint64_t r = blockIdx.x;
    const typename Elem<DT>::T* row = x + r * (uint64_t)V;
    const RowRule rule = {1.f, 1.f, 0.f};
    uint32_t thr = 0, kept;
    if (threadIdx.x == 0) n_above = 0;
    if (k < V) row_select<DT>(L, row, nullptr, V, rule, k, 1.f, thr, kept);
    __syncthreads();
    for_each_y<DT>(row, nullptr, V, rule, threadIdx.x, kSelThreads, [&](int, float y) {
        const uint32_t key = y_key(y);
        if (k >= V || key > thr) {   // < k entries (k == V: all of them)
            const uint32_t slot = atomicAdd(&n_above, 1u);
            if (slot < (uint32_t)kTopkMax) keys[slot] = key;
        }
    });
    __syncthreads();
    const int na = (int)n_above < k ? (int)n_above : k, fill = k - na;
    for (int i = threadIdx.x; i < k; i += kSelThreads) {
        uint32_t key = thr;
        int rank = i;
        if (i >= fill) {
            key = keys[i - fill];
            rank = fill;
            for (int j = 0; j < na; ++j) {
                const uint32_t o = keys[j];
                rank += (o < key || (o == key && j < i - fill)) ? 1 : 0;
            }
        }
        Elem<DT>::st(out + r * (uint64_t)k + rank, key_y(key));
    }
}

}  // namespace

int check_sampling(const char* who, const omx_sampling* p, int V) {
    OMX_REQUIRE(p, "%s: null sampling parameters", who);
    OMX_REQUIRE(p->temperature >= 0.f && p->temperature == p->temperature, "%s: temperature %f must be >= 0", who, (double)p->temperature);
    OMX_REQUIRE(p->top_k >= 0, "%s: top_k %d must be >= 0 (0 = off)", who, p->top_k);
    OMX_REQUIRE(p->top_p > 0.f && p->top_p <= 1.f, "%s: top_p %f must be in (0, 1] (1 = off)", who, (double)p->top_p);
    OMX_REQUIRE(p->repetition_penalty > 0.f && p->repetition_penalty < INFINITY, "%s: repetition_penalty %f must be positive (1 = off)", who,
                (double)p->repetition_penalty);
    OMX_REQUIRE(p->presence_penalty == p->presence_penalty && fabsf(p->presence_penalty) < INFINITY,
                "%s: presence_penalty %f must be finite (0 = off)", who, (double)p->presence_penalty);
    OMX_REQUIRE(V > 0 && V <= (1 << 23), "%s: %d entries per row (1 .. 2^23: the 64-bit fixed-point mass sums)", who, V);
    return 0;
}

namespace {

RowRule rule_of(const omx_sampling& p) {
    RowRule r;
    r.inv_temp = p.temperature == 0.f ? 1.f : 1.0f / p.temperature;
    r.rep = p.repetition_penalty;
    r.pres = p.presence_penalty;
    return r;
}

bool selects(const omx_sampling& p, int V) { return p.temperature != 0.f && ((p.top_k > 0 && p.top_k < V) || p.top_p < 1.f); }

template <int DT>
int select_launches(SelWs* ws, const typename Elem<DT>::T* row, int V, const omx_sampling& p, const uint8_t* seen, bool zero_first,
                    hipStream_t s) {
    const RowRule r = rule_of(p);
    const int k_on = p.top_k > 0 && p.top_k < V, p_on = p.top_p < 1.f;
    // the histograms start from zero: a shared scratch is cleared here, the engine's own one by the previous selection's [resolve]
    if (zero_first) OMX_HIP_CHECK(hipMemsetAsync(ws, 0, offsetof(SelWs, partials), s));
    if (p_on) select_max_kernel<DT><<<kHistBlocks, kHistThreads, 0, s>>>(ws, row, seen, V, r);
    for (int slot = 0; slot < kSlots; ++slot) {
        if ((slot == 1 || slot == 2) && !k_on) continue;
        if ((slot == 3 || slot == 4) && !p_on) continue;
        select_hist_kernel<DT><<<kHistBlocks, kHistThreads, 0, s>>>(ws, row, seen, V, r, slot, (uint32_t)p.top_k, p.top_p, k_on, p_on);
    }
    select_resolve_kernel<<<1, kHistThreads, 0, s>>>(ws, (uint32_t)p.top_k, p.top_p, V, k_on, p_on, zero_first ? 0 : 1);
    OMX_LAUNCH_CHECK();
    return 0;
}

template <int DT>
int noise_launch(unsigned long long* partials, int n_partials, const typename Elem<DT>::T* row, int V, const omx_sampling& p,
                 const uint8_t* seen, SelWs* ws, const uint32_t* sub_key, hipStream_t s) {
    sample_filtered_noise_kernel<DT><<<n_partials, 256, 0, s>>>(partials, row, seen, ws, sub_key, V, (uint64_t)V, rule_of(p),
                                                               p.temperature == 0.f);
    OMX_LAUNCH_CHECK();
    return 0;
}

// ---- the rows of a batch step, each under its own slot's rule (BatchFilterArgs, sample_filter.hpp) ----
// (state, key) = split(state, 2) of the slot's key sequence, RandomState::next: the words batch_sample_kernel derives
__device__ __forceinline__ void slot_next_key(const BatchSlot* S, uint32_t& s0, uint32_t& s1, uint32_t& k0, uint32_t& k1) {
    const uint32_t c0 = S->rng[0], c1 = S->rng[1];
    threefry2x32(c0, c1, 0u, 2u, s0, k0);
    threefry2x32(c0, c1, 1u, 3u, s1, k1);
}

// what thread 0 of a row's last block leaves: the token in the ring and as the slot's pending token, the position and (temperature != 0)
// the key sequence advanced, the token marked in the history the slot's penalties read
__device__ __forceinline__ void batch_row_advance(const BatchFilterArgs& a, int r, BatchSlot* S, unsigned long long best, bool greedy,
                                                  uint32_t s0, uint32_t s1, uint32_t k0, uint32_t k1) {
    const uint32_t token = ~(uint32_t)(best & 0xFFFFFFFFull);
    a.ring[r] = token;
    S->pending = token;
    S->pos += 1;
    if (!greedy) { S->rng[0] = s0; S->rng[1] = s1; S->rng[2] = k0; S->rng[3] = k1; }
    uint8_t* seen = a.row[r].seen;
    if (seen && token < (uint32_t)a.V) seen[token] = 1;
}

// short rows: one block per row selects (row_select), draws over the kept set and advances the slot
__global__ __launch_bounds__(kSelThreads) void batch_filtered_kernel(const BatchFilterArgs a) {
    __shared__ SelectLds L;
    __shared__ unsigned long long red[kSelThreads / 64];
    const int r = blockIdx.x, slot = a.row_slot[r], V = a.V;
    const BatchFilterRow& R = a.row[r];
    BatchSlot* S = a.slots + slot;
    const bool greedy = R.greedy != 0;
    const bf16_t* row = a.rows + (size_t)r * V;
    bf16_t* keep = a.slot_logits + (size_t)slot * V;
    const uint8_t* seen = R.seen;
    uint32_t s0 = 0, s1 = 0, k0 = 0, k1 = 0;
    if (!greedy) slot_next_key(S, s0, s1, k0, k1);
    for (int v = threadIdx.x; v < V; v += kSelThreads) keep[v] = row[v];
    uint32_t thr, kept;
    row_select<OMX_BFLOAT16>(L, row, seen, V, R.rule, greedy ? 0 : R.top_k, greedy ? 1.f : R.top_p, thr, kept);
    unsigned long long best = 0;
    for_each_y<OMX_BFLOAT16>(row, seen, V, R.rule, threadIdx.x, kSelThreads, [&](int v, float y) {
        if (y_key(y) >= thr) {
            const float g = greedy ? 0.f : gumbel_from_word(random_word(k0, k1, (uint64_t)v, (uint64_t)V));
            const unsigned long long kx = sample_key(greedy ? y : y + g, (uint32_t)v);
            best = kx > best ? kx : best;
        }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();   // every thread has read the key state and the history before thread 0 replaces them
    if (threadIdx.x == 0) {
        for (int w = 1; w < kSelThreads / 64; ++w) best = red[w] > best ? red[w] : best;
        batch_row_advance(a, r, S, best, greedy, s0, s1, k0, k1);
    }
}

// vocabulary-sized rows: the launch-per-level selection with grid.y = the row, every row on its own SelWs.  A launch is there for the
// union of the rows' settings; a row whose own settings do not need it leaves at once (the exit is uniform over the block).
__device__ __forceinline__ bool row_selects(const BatchFilterRow& R) { return !R.greedy && (R.k_on || R.p_on); }
static_assert(sizeof(SelWs) % 16 == 0, "the rows' scratch lies back to back: [resolve] clears it with 16-byte stores");
__device__ __forceinline__ SelWs* row_ws(const BatchFilterArgs& a, int r) { return (SelWs*)a.ws + r; }

__global__ __launch_bounds__(kHistThreads) void batch_select_max_kernel(const BatchFilterArgs a) {
    const int r = blockIdx.y;
    const BatchFilterRow& R = a.row[r];
    if (!row_selects(R) || !R.p_on) return;
    select_max_body<OMX_BFLOAT16>(row_ws(a, r), a.rows + (size_t)r * a.V, R.seen, a.V, R.rule);
}

__global__ __launch_bounds__(kHistThreads) void batch_select_hist_kernel(const BatchFilterArgs a, int slot) {
    const int r = blockIdx.y;
    const BatchFilterRow& R = a.row[r];
    if (!row_selects(R) || ((slot == 1 || slot == 2) && !R.k_on) || ((slot == 3 || slot == 4) && !R.p_on)) return;
    select_hist_body<OMX_BFLOAT16>(row_ws(a, r), a.rows + (size_t)r * a.V, R.seen, a.V, R.rule, slot, (uint32_t)R.top_k, R.top_p, R.k_on, R.p_on);
}

__global__ __launch_bounds__(kHistThreads) void batch_select_resolve_kernel(const BatchFilterArgs a) {
    const int r = blockIdx.y;
    const BatchFilterRow& R = a.row[r];
    if (!row_selects(R)) return;
    select_resolve_body(row_ws(a, r), (uint32_t)R.top_k, R.top_p, a.V, R.k_on, R.p_on, 1);
}

// [noise] grid (kOpPartials, M): the row kept as the slot's logits, then the partials of the draw over the kept set with the slot's NEXT key
__global__ __launch_bounds__(256) void batch_noise_kernel(const BatchFilterArgs a) {
    const int r = blockIdx.y, slot = a.row_slot[r], V = a.V;
    const BatchFilterRow& R = a.row[r];
    const bf16_t* row = a.rows + (size_t)r * V;
    bf16_t* keep = a.slot_logits + (size_t)slot * V;
    uint32_t s0 = 0, s1 = 0, k0 = 0, k1 = 0;
    if (!R.greedy) slot_next_key(a.slots + slot, s0, s1, k0, k1);
    for (int v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256) keep[v] = row[v];
    SelWs* ws = row_ws(a, r);
    filtered_noise_body<OMX_BFLOAT16>(ws->partials, row, R.seen, row_selects(R) ? ws->thr : 0u, k0, k1, V, (uint64_t)V, R.rule, R.greedy);
}

// [finalize] grid (1, M): the partials' maximum is the row's token; the slot advances
__global__ __launch_bounds__(kOpPartials) void batch_finalize_kernel(const BatchFilterArgs a) {
    __shared__ unsigned long long red[kOpPartials / 64];
    const int r = blockIdx.y;
    unsigned long long best = row_ws(a, r)->partials[threadIdx.x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kOpPartials / 64; ++w) best = red[w] > best ? red[w] : best;
        BatchSlot* S = a.slots + a.row_slot[r];
        const bool greedy = a.row[r].greedy != 0;
        uint32_t s0 = 0, s1 = 0, k0 = 0, k1 = 0;
        if (!greedy) slot_next_key(S, s0, s1, k0, k1);
        batch_row_advance(a, r, S, best, greedy, s0, s1, k0, k1);
    }
}

}  // namespace

bool sampling_filters(const omx_sampling& p, int V) { return p.repetition_penalty != 1.f || p.presence_penalty != 0.f || selects(p, V); }

BatchFilterRow batch_filter_row(const omx_sampling& p, int V, uint8_t* seen_row) {
    BatchFilterRow R = {};
    R.rule = rule_of(p);
    R.top_k = p.top_k;
    R.top_p = p.top_p;
    R.seen = seen_row;
    R.k_on = p.top_k > 0 && p.top_k < V;
    R.p_on = p.top_p < 1.f;
    R.greedy = p.temperature == 0.f;
    return R;
}

int launch_batch_filtered(const BatchFilterArgs& a, int M, hipStream_t s) {
    OMX_REQUIRE(M >= 1 && M <= kBatchFilterRows, "batch sampler: %d rows (1..%d)", M, kBatchFilterRows);
    if (a.V < kMultiLaunchMin) {
        batch_filtered_kernel<<<M, kSelThreads, 0, s>>>(a);
        OMX_LAUNCH_CHECK();
        return 0;
    }
    OMX_REQUIRE(a.ws, "batch sampler: no selection scratch");
    bool any = false, any_k = false, any_p = false;
    for (int r = 0; r < M; ++r) {
        const BatchFilterRow& R = a.row[r];
        const bool sel = !R.greedy && (R.k_on || R.p_on);
        any = any || sel;
        any_k = any_k || (sel && R.k_on);
        any_p = any_p || (sel && R.p_on);
    }
    const dim3 grid(kHistBlocks, M);
    if (any_p) batch_select_max_kernel<<<grid, kHistThreads, 0, s>>>(a);
    for (int slot = 0; slot < kSlots && any; ++slot) {
        if ((slot == 1 || slot == 2) && !any_k) continue;
        if ((slot == 3 || slot == 4) && !any_p) continue;
        batch_select_hist_kernel<<<grid, kHistThreads, 0, s>>>(a, slot);
    }
    if (any) batch_select_resolve_kernel<<<dim3(1, M), kHistThreads, 0, s>>>(a);
    batch_noise_kernel<<<dim3(kOpPartials, M), 256, 0, s>>>(a);
    batch_finalize_kernel<<<dim3(1, M), kOpPartials, 0, s>>>(a);
    OMX_LAUNCH_CHECK();
    return 0;
}

size_t sample_select_ws_bytes() { return sizeof(SelWs); }

int launch_sample_select(void* ws, const bf16_t* logits, bool logits_f16, int V, const omx_sampling& p, const uint8_t* seen,
                         hipStream_t s) {
    if (!selects(p, V)) return 0;
    return logits_f16 ? select_launches<OMX_FLOAT16>((SelWs*)ws, reinterpret_cast<const f16_t*>(logits), V, p, seen, false, s)
                      : select_launches<OMX_BFLOAT16>((SelWs*)ws, logits, V, p, seen, false, s);
}

int launch_sample_filtered_noise(unsigned long long* partials, int n_partials, const bf16_t* logits, bool logits_f16, int V,
                                 const omx_sampling& p, const uint8_t* seen, void* ws, const uint32_t* sub_key, hipStream_t s) {
    SelWs* w = selects(p, V) ? (SelWs*)ws : nullptr;
    return logits_f16 ? noise_launch<OMX_FLOAT16>(partials, n_partials, reinterpret_cast<const f16_t*>(logits), V, p, seen, w, sub_key, s)
                      : noise_launch<OMX_BFLOAT16>(partials, n_partials, logits, V, p, seen, w, sub_key, s);
}

int launch_mark_seen(uint8_t* seen, int V, const StepState* st, hipStream_t s) {
    mark_seen_kernel<<<1, 1, 0, s>>>(seen, V, st);
    OMX_LAUNCH_CHECK();
    return 0;
}

}  // namespace omx

extern "C" {

int omx_sample_filtered(uint32_t* out_token, const void* logits, omx_dtype dtype, int64_t rows, int V, const omx_sampling* p,
                        const uint8_t* seen, const uint32_t* key, float* thr_out, int32_t* kept_out, omx_stream stream) {
    OMX_REQUIRE(out_token && logits, "omx_sample_filtered: null tensor");
    if (omx::check_sampling("omx_sample_filtered", p, V)) return 1;
    const int greedy = p->temperature == 0.f;
    OMX_REQUIRE(greedy || key, "omx_sample_filtered: a key is needed at temperature %f", (double)p->temperature);
    OMX_REQUIRE(rows >= 0 && rows <= 0x7FFFFFFFLL, "omx_sample_filtered: too many rows");
    if (rows == 0) return 0;
    const uint64_t words = (uint64_t)rows * (uint64_t)V;
    OMX_REQUIRE(words <= 0x1FFFFFFFEULL, "omx_sample_filtered: %llu noise words exceed the counter space of one key", (unsigned long long)words);
    if (rows == 1 && V >= omx::kMultiLaunchMin && omx::selects(*p, V)) {   // a vocabulary-sized row: the selection over many blocks
        void* ws = nullptr;
        if (omx::get_workspace(&ws, sizeof(omx::SelWs))) return 1;
        omx::SelWs* w = (omx::SelWs*)ws;
        hipStream_t s = (hipStream_t)stream;
        OMX_DISPATCH_FLOAT(dtype, "omx_sample_filtered",
                           if (omx::select_launches<DT>(w, (const omx::Elem<DT>::T*)logits, V, *p, seen, true, s) ||
                               omx::noise_launch<DT>(w->partials, omx::kOpPartials, (const omx::Elem<DT>::T*)logits, V, *p, seen, w, key, s))
                               return 1);
        omx::select_finish_kernel<<<1, omx::kOpPartials, 0, s>>>(out_token, thr_out, kept_out, w);
        OMX_LAUNCH_CHECK();
        return 0;
    }
    const omx::RowRule r = omx::rule_of(*p);
    OMX_DISPATCH_FLOAT(dtype, "omx_sample_filtered",
                       (omx::sample_filtered_kernel<DT><<<(unsigned)rows, omx::kSelThreads, 0, (hipStream_t)stream>>>(
                           out_token, (const omx::Elem<DT>::T*)logits, seen, key, V, words, r, p->top_k, p->top_p, greedy, thr_out, kept_out)));
    OMX_LAUNCH_CHECK();
    return 0;
}

int omx_topk_values(void* out, const void* x, omx_dtype dtype, int64_t rows, int V, int k, omx_stream stream) {
    OMX_REQUIRE(out && x, "omx_topk_values: null tensor");
    OMX_REQUIRE(V > 0 && V <= (1 << 23), "omx_topk_values: %d entries per row (1 .. 2^23)", V);
    OMX_REQUIRE(k >= 1 && k <= V, "omx_topk_values: k=%d must be in 1 .. %d", k, V);
    OMX_REQUIRE(k <= omx::kTopkMax, "omx_topk_values: k=%d exceeds the %d values one block orders in LDS", k, omx::kTopkMax);
    OMX_REQUIRE(rows >= 0 && rows <= 0x7FFFFFFFLL, "omx_topk_values: too many rows");
    if (rows == 0) return 0;
    OMX_DISPATCH_FLOAT(dtype, "omx_topk_values",
                       (omx::topk_values_kernel<DT><<<(unsigned)rows, omx::kSelThreads, 0, (hipStream_t)stream>>>(
                           (omx::Elem<DT>::T*)out, (const omx::Elem<DT>::T*)x, V, k)));
    OMX_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
