// Long-sequence float32 attention at head width 64 on v_mfma_f32_16x16x4_f32, the online-softmax form: no score of a row outlives its
// 64-key chunk, so the key count is unbounded (the score-in-LDS kernels -- vit_attn_kernel, attn_f32.hip -- stop at 1024 keys).  Three
// users, one text (sam_encoder.hip, vcf_encoder.hip):
//   SA_GLOBAL  a SAM global block: all gh * gw keys of an image, + the decomposed relative-position bias
//   SA_WINDOW  a SAM window block: the grid zero-padded to multiples of the window and cut into windows; a block's keys are one window's
//              win * win positions, read IN PLACE from the image-order rows, padded positions reading the padded token's q | k | v row
//   SA_PREFIX  the visual-causal-flow mask over GQA heads: row i sees keys j < max(n_prefix, i + 1); no bias
// Block = (64 query rows of one domain, query head), four waves, wave w owning rows 16 w .. 16 w + 15 from the scores to the output -- no
// reduction crosses a wave.  Everything is computed TRANSPOSED so that a query sits on lane & 15 in all three products' layouts:
//   S^T = K . Q^T    A = K fragment from LDS (lane (n, g): key n, dims 8 j + 2 g, + 1 -- the permuted term order of vit_attn_kernel, two
//                    accumulator chains), B = the wave's Q fragments, held in registers for the whole pass.  D: key 4 g + r, query n.
//   softmax          running maximum m and sum l per query; a query's 16 scores of a chunk lie in 4 registers x 4 lane groups: two
//                    xor-shuffles (16, 32).  Masked scores are -inf; every row sees key 0, so m is finite from the first chunk on.
//   O^T = V^T . P^T  the MFMA step (tile t, register r) sums over the keys 16 t + 4 g + r, g = 0 .. 3: lane (n, g) supplies ITS OWN
//                    p register as B and V[that key][16 c + n] from LDS as A -- P never moves between lanes.  D: dim 16 c + 4 g + r,
//                    query n, rescaled by exp(m_old - m_new) per chunk, divided by l at the end.
// K and V chunks (64 keys x 64 dims each) are staged global -> registers -> LDS by all 256 threads (16-byte loads of whole rows; the next
// chunk's loads are in flight while this one is computed); LDS rows of 68 floats: the 8-byte K fragment reads and the 4-byte V fragment
// reads are conflict-free.  Keys at and past the domain's end are staged as zeros and masked.
// The bias s += q . Rh[qh, kh] + q . Rw[qw, kw] (unscaled q) never exists as [N, N]: at entry the block computes its 64 rows'
// q . T_h[row(qh - kh + gh - 1)] for the gh values of kh and likewise the gw values of kw into LDS ([64][gh + gw], 32 KiB at 64 x 64) --
// plain fmaf chains in dimension order, q in registers, the table row wave-uniform.  The resampling of a table whose length is not
// 2 g - 1 (vision.rs:186-196) is an index computed in place.
// One fixed order of every sum: the same input gives the same bits.
#pragma once
#include <math.h>

#include "common.hpp"

namespace omx {

enum { SA_GLOBAL = 0, SA_WINDOW = 1, SA_PREFIX = 2 };
constexpr int SA_Q = 64, SA_KC = 64, SA_LD = 68;
using sa_f32x2 = __attribute__((ext_vector_type(2))) float;

struct StreamAttn {
    const float* qkv;          // rows of the stacked projection, `images` images of n rows each
    const float* pad;          // SA_WINDOW: the padded token's q | k | v row (same column layout), null when nothing is padded
    float* out;                // [images * n, heads * 64] rows ldo floats apart
    int64_t ld, ldo;
    int qoff, koff, voff;      // first column of q / k / v
    int heads, group;          // query heads; query heads per key/value head
    int n;                     // rows of an image
    int dom;                   // rows of a domain: n, or win * win
    int gh, gw, win, nwx, nwy; // the grid; SA_WINDOW: the window and the windows per axis
    int ph, pw;                // the domain's own grid: gh x gw, or win x win
    int n_prefix;
    const float* th; const float* tw;   // rel_pos_h [Lh, 64], rel_pos_w [Lw, 64]
    int Lh, Lw;
    float sh, sw;              // Lh / (2 ph - 1) in float32 where the table is resampled, 0 where it is exact
    float scale;
};

inline size_t sa_lds_bytes(int mode, int ph, int pw) {
    return ((size_t)2 * SA_KC * SA_LD + (mode == SA_PREFIX ? 0 : (size_t)SA_Q * ((ph + pw) | 1))) * sizeof(float);
}

// the q | k | v row of position idx of domain dz (null: SA_WINDOW, a padded position and no pad row -- the launcher refuses that case)
template <int MODE>
__device__ __forceinline__ int64_t sa_row(const StreamAttn& a, int dz, int idx) {
    if (MODE != SA_WINDOW) return (int64_t)dz * a.n + idx;
    const int nwin = a.nwx * a.nwy, img = dz / nwin, w = dz % nwin;
    const int y = (w / a.nwx) * a.win + idx / a.win, x = (w % a.nwx) * a.win + idx % a.win;
    return (y < a.gh && x < a.gw) ? (int64_t)img * a.n + (int64_t)y * a.gw + x : (int64_t)-1;
}

template <int MODE>
__global__ __launch_bounds__(256) void stream_attn_kernel(const StreamAttn a) {
    extern __shared__ __attribute__((aligned(16))) float sa_lds[];
    float* Ks = sa_lds;                                // [64 keys][68]
    float* Vs = Ks + SA_KC * SA_LD;                    // [64 keys][68]
    float* Bq = Vs + SA_KC * SA_LD;                    // [64 rows][bld]: q . T_h for kh = 0 .. ph - 1, then q . T_w for kw = 0 .. pw - 1
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int head = blockIdx.y, hk = (head / a.group) * 64, dz = blockIdx.z, q0 = blockIdx.x * SA_Q, N = a.dom;
    const int bld = (a.ph + a.pw) | 1;
    auto row_ptr = [&](int idx) -> const float* {
        const int64_t r = sa_row<MODE>(a, dz, idx);
        return r < 0 ? a.pad : a.qkv + r * a.ld;
    };

    if (MODE != SA_PREFIX) {
        // thread (row r = t & 63, quarter t >> 6): its row's q in registers, table rows j = quarter, quarter + 4, ...
        const int r = threadIdx.x & 63, idx = min(q0 + r, N - 1), py = idx / a.pw, px = idx % a.pw;
        const float* qr = row_ptr(idx) + a.qoff + head * 64;
        f32x4 qv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) qv[i] = *reinterpret_cast<const f32x4*>(qr + 4 * i);
        for (int j = wave; j < a.ph + a.pw; j += 4) {
            const bool isw = j >= a.ph;
            const int rel = isw ? px - (j - a.ph) + (a.pw - 1) : py - j + (a.ph - 1);
            const int L = isw ? a.Lw : a.Lh;
            const float sc = isw ? a.sw : a.sh;
            const int trow = sc != 0.f ? min((int)((float)rel * sc), L - 1) : rel;
            const float* tr = (isw ? a.tw : a.th) + (int64_t)trow * 64;
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(tr + 4 * i);
                acc = fmaf(qv[i][0], t[0], acc); acc = fmaf(qv[i][1], t[1], acc); acc = fmaf(qv[i][2], t[2], acc); acc = fmaf(qv[i][3], t[3], acc);
            }
            Bq[r * bld + j] = acc;
        }
    }

    const int myrow = q0 + 16 * wave + n, qidx = min(myrow, N - 1);
    const bool wave_on = q0 + 16 * wave < N;
    sa_f32x2 qf[8];
    {
        const float* qr = row_ptr(qidx) + a.qoff + head * 64 + 2 * g;
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[j] = *reinterpret_cast<const sa_f32x2*>(qr + 8 * j);
    }
    const int lim = MODE == SA_PREFIX ? max(a.n_prefix, qidx + 1) : N;
    const int kend = MODE == SA_PREFIX ? min(N, max(a.n_prefix, q0 + SA_Q)) : N;
    const float* brow = Bq + (16 * wave + n) * bld;

    float m = -INFINITY, l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (f32x4){0.f, 0.f, 0.f, 0.f};

    f32x4 kreg[4], vreg[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + 256 * i, key = k0 + (e >> 4), c4 = (e & 15) * 4;
            kreg[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            vreg[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (key < N) {
                const float* p = row_ptr(key);
                kreg[i] = *reinterpret_cast<const f32x4*>(p + a.koff + hk + c4);
                vreg[i] = *reinterpret_cast<const f32x4*>(p + a.voff + hk + c4);
            }
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < kend; k0 += SA_KC) {
        __syncthreads();                               // the chunk before is read (first pass: the bias table is written)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + 256 * i;
            *reinterpret_cast<f32x4*>(Ks + (e >> 4) * SA_LD + (e & 15) * 4) = kreg[i];
            *reinterpret_cast<f32x4*>(Vs + (e >> 4) * SA_LD + (e & 15) * 4) = vreg[i];
        }
        __syncthreads();
        if (k0 + SA_KC < kend) fetch(k0 + SA_KC);
        if (!wave_on) continue;
        const int tiles = min(4, (kend - k0 + 15) / 16);
        f32x4 s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (t < tiles) {
                const float* kr = Ks + (16 * t + n) * SA_LD + 2 * g;
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const sa_f32x2 kf = *reinterpret_cast<const sa_f32x2*>(kr + 8 * j);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[0], qf[j][0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[1], qf[j][1], acc1, 0, 0, 0);
                }
                // the key's place in the domain's grid: one division per tile, then steps of one key
                int ky = 0, kx = 0;
                if (MODE != SA_PREFIX) { ky = (k0 + 16 * t + 4 * g) / a.pw; kx = (k0 + 16 * t + 4 * g) % a.pw; }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = k0 + 16 * t + 4 * g + r;
                    float v = (acc0[r] + acc1[r]) * a.scale;
                    if (MODE != SA_PREFIX) {
                        v += brow[min(ky, a.ph - 1)] + brow[a.ph + kx];       // (keys past the end: any finite entry, masked below)
                        if (++kx == a.pw) { kx = 0; ++ky; }
                    }
                    s[t][r] = key < lim ? v : -INFINITY;
                }
            }
        }
        float cm = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) cm = fmaxf(cm, s[t][r]);
        cm = fmaxf(cm, __shfl_xor(cm, 16));
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        const float mn = fmaxf(m, cm);                 // finite: key 0 is visible to every row
        const float alpha = expf(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) { s[t][r] = expf(s[t][r] - mn); ps += s[t][r]; }
        ps += __shfl_xor(ps, 16);
        ps += __shfl_xor(ps, 32);
        l = l * alpha + ps;
        m = mn;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] *= alpha;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < tiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* vr = Vs + (16 * t + 4 * g + r) * SA_LD + n;
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[16 * c], s[t][r], o[c], 0, 0, 0);
                }
            }
        }
    }
    if (!wave_on || myrow >= N) return;
    const int64_t orow = sa_row<MODE>(a, dz, myrow);
    if (orow < 0) return;                              // a padded position's query row is dropped
    float* op = a.out + orow * a.ldo + head * 64 + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) *reinterpret_cast<f32x4*>(op + 16 * c) = o[c] / l;
}

// images: how many images are stacked; domains per image = 1 or nwx * nwy
inline int launch_stream_attn(int mode, const StreamAttn& a, int images, hipStream_t s) {
    const size_t lds = sa_lds_bytes(mode, a.ph, a.pw);
    OMX_REQUIRE(lds <= (size_t)160 * 1024, "InvalidConfig: attention: a %d x %d grid needs %zu bytes of LDS for its bias table (at most 160 KiB)", a.ph, a.pw, lds);
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    OMX_REQUIRE(a.ld % 4 == 0 && a.ldo % 4 == 0 && a.qoff % 4 == 0 && a.koff % 4 == 0 && a.voff % 4 == 0 && al16(a.qkv) && al16(a.out) && al16(a.pad) &&
                al16(a.th) && al16(a.tw), "attention: rows must be 16-byte aligned (ld %lld, ldo %lld)", (long long)a.ld, (long long)a.ldo);
    const int doms = mode == SA_WINDOW ? a.nwx * a.nwy : 1;
    OMX_REQUIRE((int64_t)images * doms <= 65535, "InvalidConfig: attention: %d images of %d windows exceed one launch's 65535 domains", images, doms);
    const dim3 grid((a.dom + SA_Q - 1) / SA_Q, a.heads, images * doms);
    const void* fn = mode == SA_GLOBAL ? (const void*)stream_attn_kernel<SA_GLOBAL> : mode == SA_WINDOW ? (const void*)stream_attn_kernel<SA_WINDOW>
                                                                                                         : (const void*)stream_attn_kernel<SA_PREFIX>;
    if (lds > 64 * 1024) OMX_REQUIRE(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess,
                                     "attention: the device refused %zu bytes of LDS per block", lds);
    if (mode == SA_GLOBAL) stream_attn_kernel<SA_GLOBAL><<<grid, 256, lds, s>>>(a);
    else if (mode == SA_WINDOW) stream_attn_kernel<SA_WINDOW><<<grid, 256, lds, s>>>(a);
    else stream_attn_kernel<SA_PREFIX><<<grid, 256, lds, s>>>(a);
    OMX_LAUNCH_CHECK();
    return 0;
}

}  // namespace omx
