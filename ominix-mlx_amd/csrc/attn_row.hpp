// The per-row arithmetic of a split of split-KV decode attention (Tq == 1), written once: what a (row, KV head, split) partial is, to
// the bit.  attn_decode_kernel (attn_decode.hip: the per-op decode SDPA and the rows of a speculative verify pass) and
// batch_attn_kernel / batch_attn_shared_kernel (engine_batch.hip) are built from it; they differ in where a row's query, K/V and token
// range come from (a source policy: bf16 rows, or the 8-bit affine rows of a kv_bits = 8 batch), and in the mask.
//
// Mapping (wave64, blocks of kBlock threads = kWaves waves): K/V rows are D bf16 = D/8 lanes x 16 B straight to registers, so a
// wave-instruction covers 64/(D/8) consecutive tokens as one contiguous 1 KiB burst; the G = H/Hkv query heads of a KV head are
// processed together in registers, so each K/V byte is read once per KV head (GQA without tiling, fast.rs:118); scores are a per-lane
// 8-element partial dot reduced over the D/8-lane group with DPP row ops; softmax state (m, l) in fp32 (fast.rs:116), ONE running max
// per head and wave (v_readlane across its token sub-groups) so that sub-group partials merge by plain sums; the waves' partials are
// merged through LDS into an un-normalised (m, l, o[D]) per head and split, which the caller's merge kernel combines.
#pragma once
#include "common.hpp"

namespace omx {

constexpr int kBlock = 256;
constexpr int kWaves = 4;
constexpr int kUnroll = 4;   // token rows per lane-group per step -> 4 K + 4 V loads in flight

__device__ __forceinline__ void unpack8(const u32x4 r, float (&x)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        x[2 * e] = bf16lo(r[e]);
        x[2 * e + 1] = bf16hi(r[e]);
    }
}

// Where a split's K/V rows come from: how the 8 elements (chunk c) a lane owns of token row tc of a KV head are issued, what stays in
// registers until they are used (Raw), and how they unpack to fp32.  bf16 rows [tokens, D]: one 16-byte load each
struct KvBf16 {
    typedef u32x4 Raw;
    const bf16_t *K, *V;
    template <int D>
    __device__ __forceinline__ void issue(Raw& k, Raw& v, int tc, int c) const {
        k = *reinterpret_cast<const u32x4*>(K + (size_t)tc * D + c * 8);
        v = *reinterpret_cast<const u32x4*>(V + (size_t)tc * D + c * 8);
    }
    static __device__ __forceinline__ void unpack(const Raw& r, float (&x)[8]) { unpack8(r, x); }
};
// 8-bit MLX affine rows (group 64 along the head dim): codes [tokens, D] bytes, one word scale | bias (bf16 low | high) per group
// [tokens, D / 64] -- an 8-byte load plus the word of the lane's group; element = (float)code * scale + bias, never rounded to bf16
struct Kv8Raw {
    u32x2 q;
    uint32_t sb;
};
struct KvAffine8 {
    typedef Kv8Raw Raw;
    const uint8_t *K, *V;
    const uint32_t *Ksb, *Vsb;
    template <int D>
    __device__ __forceinline__ void issue(Raw& k, Raw& v, int tc, int c) const {
        k.q = *reinterpret_cast<const u32x2*>(K + (size_t)tc * D + c * 8);
        v.q = *reinterpret_cast<const u32x2*>(V + (size_t)tc * D + c * 8);
        k.sb = Ksb[(size_t)tc * (D / 64) + c / 8];
        v.sb = Vsb[(size_t)tc * (D / 64) + c / 8];
    }
    static __device__ __forceinline__ void unpack(const Raw& r, float (&x)[8]) {
        const float sc = bf16lo(r.sb), b = bf16hi(r.sb);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = fmaf((float)((r.q[e >> 2] >> (8 * (e & 3))) & 0xFFu), sc, b);
    }
};

// scores()'s mask hook: score d of token tok as it enters the softmax; live = the token lies inside the split's range (the others
// score -inf whatever the hook returns, and a mask is not read for them).  No mask: as it is
struct NoMask {
    __device__ __forceinline__ float operator()(float d, int, bool) const { return d; }
};

// A lane owns 8 elements (c) of the head dim of token sub-group sg of its wave.
template <int D, int GT>
struct AttnRow {
    static constexpr int LPR = D / 8;          // lanes per K/V row
    static constexpr int TPW = 64 / LPR;       // tokens per wave-instruction == token sub-groups per wave
    static constexpr int STEP = TPW * kUnroll; // tokens per wave per step
    // the block's LDS, what finish() merges through: [kWaves][TPW][GT][D] o, [kWaves][GT] m, [kWaves][GT] l (+ 4 floats of slack)
    static constexpr int SM_O = kWaves * TPW * GT * D, SM_ML = kWaves * GT;
    static constexpr size_t SMEM_BYTES = (size_t)(SM_O + 2 * SM_ML + 4) * sizeof(float);
    float q[GT][8], m[GT], l[GT], o[GT][8];

    // the wave's STEP K and V rows from token tbase on, of a head whose rows start at Kb / Vb (row stride D); rows past the split's
    // end are clamped duplicates
    template <class Src>
    static __device__ __forceinline__ void issue_rows(typename Src::Raw (&kr)[kUnroll], typename Src::Raw (&vr)[kUnroll], const Src& src,
                                                      int tbase, int t_end, int sg, int c) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int tc = max(min(tbase + u * TPW + sg, t_end - 1), 0);
            src.template issue<D>(kr[u], vr[u], tc, c);
        }
    }
    static __device__ __forceinline__ void issue_kv(u32x4 (&kr)[kUnroll], u32x4 (&vr)[kUnroll], const bf16_t* Kb, const bf16_t* Vb,
                                                    int tbase, int t_end, int sg, int c) {
        issue_rows(kr, vr, KvBf16{Kb, Vb}, tbase, t_end, sg, c);
    }

    // the G query heads of KV head kvh -> registers, pre-multiplied by scale in fp32; head h of the row at qrow + h * q_hs
    __device__ __forceinline__ void begin(const bf16_t* qrow, int64_t q_hs, float scale, int kvh, int G, int c) {
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            const int h = kvh * G + min(g, G - 1);
            float x[8];
            unpack8(*reinterpret_cast<const u32x4*>(qrow + (size_t)h * q_hs + c * 8), x);
#pragma unroll
            for (int e = 0; e < 8; ++e) q[g][e] = x[e] * scale;
        }
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            m[g] = -INFINITY;
            l[g] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
        }
    }

    // scores of the wave's STEP tokens from t0 on against the K rows in kr, each through the mask hook; the V rows unpacked
    // (Src: the rows' source, KvBf16 / KvAffine8)
    template <class Src, class Mask>
    __device__ __forceinline__ void scores_of(const typename Src::Raw (&kr)[kUnroll], const typename Src::Raw (&vr)[kUnroll], int t0, int t_end,
                                              int sg, const Mask& mask, float (&s)[kUnroll][GT], float (&vf)[kUnroll][8]) const {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int tok = t0 + u * TPW + sg;
            float kf[8];
            Src::unpack(kr[u], kf);
            Src::unpack(vr[u], vf[u]);
            if (tok >= t_end) {   // clamped duplicate row: its p is 0, but 0 * garbage must stay 0
#pragma unroll
                for (int e = 0; e < 8; ++e) vf[u][e] = 0.f;
            }
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) d = fmaf(q[g][e], kf[e], d);
                d = group_sum<LPR>(d);
                d = mask(d, tok, tok < t_end);
                s[u][g] = tok < t_end ? d : -INFINITY;
            }
        }
    }

    template <class Mask>
    __device__ __forceinline__ void scores(const u32x4 (&kr)[kUnroll], const u32x4 (&vr)[kUnroll], int t0, int t_end, int sg,
                                           const Mask& mask, float (&s)[kUnroll][GT], float (&vf)[kUnroll][8]) const {
        scores_of<KvBf16>(kr, vr, t0, t_end, sg, mask, s, vf);
    }

    // running max / sum / output of the wave over those tokens
    __device__ __forceinline__ void update(const float (&s)[kUnroll][GT], const float (&vf)[kUnroll][8]) {
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            float mx = s[0][g];
#pragma unroll
            for (int u = 1; u < kUnroll; ++u) mx = fmaxf(mx, s[u][g]);
            float wmx = readlane_f(mx, 0);
#pragma unroll
            for (int rr = 1; rr < TPW; ++rr) wmx = fmaxf(wmx, readlane_f(mx, rr * LPR));
            const float mn = fmaxf(m[g], wmx);
            const float alpha = (mn == -INFINITY) ? 1.f : __expf(m[g] - mn);
            m[g] = mn;
            l[g] *= alpha;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[g][e] *= alpha;
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const float p = (mn == -INFINITY) ? 0.f : __expf(s[u][g] - mn);
                l[g] += p;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[g][e] = fmaf(p, vf[u][e], o[g][e]);
            }
        }
    }

    // every token sub-group parks its partial in LDS (same m inside a wave: plain sums; the LPR lanes of a sub-group hold identical l);
    // the 4 waves x TPW sub-groups are merged and the split's partial written: head head0 + g to ws_o [head][nsplit][D] and ws_ml
    // [head][nsplit][2], nsplit the workspace's splits per head
    __device__ __forceinline__ void finish(unsigned char* smem, float* ws_o, float* ws_ml, int nsplit, size_t head0, int G, int split) const {
        float* sm_o = reinterpret_cast<float*>(smem);
        float* sm_m = sm_o + SM_O;
        float* sm_l = sm_m + SM_ML;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int c = lane % LPR, sg = lane / LPR;
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            float* dst = sm_o + (((size_t)(wave * TPW + sg) * GT + g) * D + c * 8);
            *reinterpret_cast<f32x4*>(dst) = f32x4{o[g][0], o[g][1], o[g][2], o[g][3]};
            *reinterpret_cast<f32x4*>(dst + 4) = f32x4{o[g][4], o[g][5], o[g][6], o[g][7]};
            float lw = readlane_f(l[g], 0);
#pragma unroll
            for (int rr = 1; rr < TPW; ++rr) lw += readlane_f(l[g], rr * LPR);
            if (lane == 0) {
                sm_m[wave * GT + g] = m[g];
                sm_l[wave * GT + g] = lw;
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < G * D; idx += kBlock) {
            const int g = idx / D, d = idx % D;
            float M = sm_m[g];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) M = fmaxf(M, sm_m[w * GT + g]);
            float L = 0.f, O = 0.f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const float mw = sm_m[w * GT + g];
                const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
                float ow = 0.f;
#pragma unroll
                for (int rr = 0; rr < TPW; ++rr) ow += sm_o[((size_t)(w * TPW + rr) * GT + g) * D + d];
                L = fmaf(f, sm_l[w * GT + g], L);
                O = fmaf(f, ow, O);
            }
            const size_t head = head0 + g;
            ws_o[(head * nsplit + split) * D + d] = O;
            if (d == 0) {
                ws_ml[(head * nsplit + split) * 2] = M;
                ws_ml[(head * nsplit + split) * 2 + 1] = L;
            }
        }
    }
};

}  // namespace omx
