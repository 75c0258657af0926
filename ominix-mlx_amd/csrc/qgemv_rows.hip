// Packed-weight (MLX affine 2/3/4/5/6/8-bit) GEMV over a HANDFUL of activation rows (M <= 8): the speculative verify pass of a quantized
// checkpoint.  launch_qgemv with n_batch = M puts the rows on grid.y and so streams the packed weights once PER ROW; here every packed
// word and scale / bias group is read from HBM once per launch, whatever M is, and multiplied against all M rows.
//
// Numerics contract: out[t, :] is bit-identical to launch_qgemv's VALU kernel (quant.hip qgemv_kernel, no matrix-core tiles) on row t.
// Each lane keeps that kernel's element assignment (lane chunk = step * 64 + lane, EPL elements), its per-step group arithmetic
// (d = ordered dot of the chunk, acc = fma(scale, d, acc), acc = fma(bias', sum(x of the chunk), acc)), its wave reduction and its
// epilogues; only the loop over the rows moves inside.  The activation rows are staged in LDS with the same per-chunk sums (and the same
// RMSNorm prologue arithmetic), one set per row, in K chunks of kc_max(MT) elements so that eight rows of the down projection
// (K = 12288) fit.
//   block = 4 waves; a wave owns RB logical rows (4, or 2 gate / up pairs for SwiGLU = 4 physical rows) and, when K is staged in one
//   chunk, `nb` consecutive such batches (the vocabulary matrix: 16 rows per wave, the activation staged once per 64 rows).  Per step a
//   lane loads the W words of its chunk of each of the 4 rows (non-temporal, two steps in flight), unpacks each row ONCE and multiplies
//   the unpacked operands against every staged row: VALU per 16 bytes of weights = unpack + M x the single-row dot products.
#include "quant.hpp"
#include "act16.hpp"
#include "gemv_parts.hpp"
#include "launch_timing.hpp"

namespace omx {
namespace {

// elements of K staged per chunk for MT rows: MT x kc x 2 bytes of bf16 = 64 KB (+ the chunk sums)
constexpr int kc_max(int MT) { return MT <= 2 ? 16384 : MT <= 4 ? 8192 : 4096; }

template <int BITS, int W, int PRO, int EPI, int MT, bool SB>
__global__ __launch_bounds__(256) void qgemv_rows_kernel(const QRowsArgs ra) {
    const QGemvArgs& a = ra.g;
    typedef Act16<false> A16;
    constexpr bool CH = quant_chunked(BITS);
    static_assert(!CH || W == BITS, "a chunked width streams one run of BITS words per lane and step");
    constexpr int EPW = 32 / BITS, EPL = CH ? 32 : W * EPW;          // elements per lane per step
    static_assert(EPL >= 8, "a lane chunk must cover at least one 16-byte activation vector");
    constexpr int LR = (EPI == EPI_SWIGLU) ? 2 : 1;                  // physical rows per logical row
    constexpr int RB = (EPI == EPI_SWIGLU) ? 2 : 4;                  // logical rows per batch
    constexpr int NR = RB * LR;
    constexpr int KCM = kc_max(MT);
    constexpr bool DOT2 = BITS != 8;                                 // 8 bits: fma on the unpacked byte, as the single-row kernel
    constexpr int NOP = DOT2 ? EPL / 2 : EPL;                        // unpacked operands per row and step
    extern __shared__ __attribute__((aligned(16))) unsigned char qrows_smem[];
    const int K = a.K, N = a.N, M = ra.M;
    const int KC = K <= KCM ? K : KCM;                               // staged elements per chunk (a multiple of 64 * EPL when K > KCM)
    bf16_t* xs = reinterpret_cast<bf16_t*>(qrows_smem);                              // [MT][KC]
    float* xsum = reinterpret_cast<float*>(qrows_smem + (size_t)MT * KC * 2);         // [MT][KC / EPL]
    float* red = xsum + MT * (KC / EPL);                                              // [8]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    const int steps = CH ? (K + 64 * EPL - 1) / (64 * EPL) : K / (64 * EPL);
    const int nchunks = K / EPL;
    const int spc = K <= KCM ? steps : KCM / (64 * EPL);              // steps per staged K chunk
    const int words_per_row = CH ? K / 32 * BITS : K / EPW, groups_per_row = K / a.group;
    const int nb = ra.nb;                                             // batches per wave (> 1 only with one staged chunk)
    const int row_base = (blockIdx.x * 4 + wave) * RB * nb;
    const int nunits = nb * steps;

    auto locate = [&](int pr, const uint32_t*& wq, const bf16_t*& sc, const bf16_t*& bi, const uint32_t*& sbp) {
        int mi, row;
        if (EPI == EPI_SWIGLU) {
            mi = pr & 1;
            row = min(pr >> 1, N - 1);
        } else {
            row = min(pr, N - 1);
            mi = 0;
            if (row >= a.m[0].n) { row -= a.m[0].n; mi = 1; if (row >= a.m[1].n) { row -= a.m[1].n; mi = 2; } }
        }
        const QMat& Mm = a.m[mi];
        wq = Mm.w + (size_t)row * words_per_row;
        sc = Mm.scales + (size_t)row * groups_per_row;
        bi = Mm.biases ? Mm.biases + (size_t)row * groups_per_row : nullptr;
        sbp = SB ? Mm.sb + (size_t)row * groups_per_row : nullptr;
    };
    struct Unit {
        uint32_t wd[NR][W];
        bf16_t sc[NR], bi[NR];
        uint32_t sbv[NR];
    };
    const uint32_t* rw[NR];
    const bf16_t* rs[NR];
    const bf16_t* rb[NR];
    const uint32_t* rsb[NR];
    auto issue = [&](Unit& u, int f) {
        const int st = f % steps;
        if (st == 0) {
            const int r0 = row_base + (f / steps) * RB;
#pragma unroll
            for (int r = 0; r < NR; ++r) locate(EPI == EPI_SWIGLU ? 2 * (r0 + r / 2) + (r & 1) : r0 + r, rw[r], rs[r], rb[r], rsb[r]);
        }
        const int chunk = st * 64 + lane;
        const int g = chunk * EPL / a.group;
        if constexpr (CH) {
            if (chunk >= nchunks) return;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint32_t* p = rw[r] + (size_t)chunk * W;
            if constexpr (CH) {
                typedef uint32_t v4a __attribute__((ext_vector_type(4), aligned(4)));
                typedef uint32_t v3a __attribute__((ext_vector_type(3), aligned(4)));
                typedef uint32_t v2a __attribute__((ext_vector_type(2), aligned(4)));
                if (W == 2) {
                    const v2a v = __builtin_nontemporal_load(reinterpret_cast<const v2a*>(p));
                    u.wd[r][0] = v[0]; u.wd[r][W > 1 ? 1 : 0] = v[1];
                } else if (W == 3) {
                    const v3a v = __builtin_nontemporal_load(reinterpret_cast<const v3a*>(p));
#pragma unroll
                    for (int k = 0; k < 3; ++k) u.wd[r][k < W ? k : 0] = v[k];
                } else {
                    const v4a v = __builtin_nontemporal_load(reinterpret_cast<const v4a*>(p));
#pragma unroll
                    for (int k = 0; k < 4; ++k) u.wd[r][k < W ? k : 0] = v[k];
                    if (W == 5) {
                        u.wd[r][W > 4 ? 4 : 0] = __builtin_nontemporal_load(p + 4);
                    } else {
                        const v2a t = __builtin_nontemporal_load(reinterpret_cast<const v2a*>(p + 4));
                        u.wd[r][W > 4 ? 4 : 0] = t[0]; u.wd[r][W > 5 ? 5 : 0] = t[1];
                    }
                }
            } else if (W == 4) {
                const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
                u.wd[r][0] = v[0]; u.wd[r][W > 1 ? 1 : 0] = v[1]; u.wd[r][W > 2 ? 2 : 0] = v[2]; u.wd[r][W > 3 ? 3 : 0] = v[3];
            } else if (W == 2) {
                const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
                u.wd[r][0] = v[0]; u.wd[r][W > 1 ? 1 : 0] = v[1];
            } else {
                u.wd[r][0] = __builtin_nontemporal_load(p);
            }
            if (SB) {
                u.sbv[r] = rsb[r][g];
            } else {
                u.sc[r] = rs[r][g];
                u.bi[r] = rb[r] ? rb[r][g] : (bf16_t)0;
            }
        }
    };

    // RMSNorm prologue: every row's 1 / rms over the WHOLE row first (the single-row kernel's sums: thread t adds the squares of
    // elements [8 t + 2048 j, +8) for j = 0.. in order, then block_sum<4>), the staging below normalises chunk by chunk
    float rstd[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) rstd[t] = 0.f;
    auto stage = [&](int c) {
        const int k0 = c * KC, kc = min(KC, K - k0);
        __syncthreads();                                                 // the previous chunk's reads are done
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            if (t >= M) break;
            const bf16_t* xg = a.x + (size_t)t * K + k0;
            bf16_t* xst = xs + (size_t)t * KC;
            float* xsm = xsum + t * (KC / EPL);
            auto put = [&](int i, const u32x4 o) { stage_chunk<A16, EPL, BITS == 4>(xst, xsm, i, o); };   // on row t's chunk
            constexpr int NV = KCM / 2048;                               // 16-byte vectors per thread and chunk (all in flight at once)
            u32x4 v[NV], nwv[NV];
#pragma unroll
            for (int it = 0; it < NV; ++it) {
                const int i = threadIdx.x * 8 + it * 2048;
                if (i < kc) {
                    v[it] = *reinterpret_cast<const u32x4*>(xg + i);
                    if (PRO == PRO_RMSNORM) nwv[it] = *reinterpret_cast<const u32x4*>(a.norm_w + k0 + i);
                }
            }
#pragma unroll
            for (int it = 0; it < NV; ++it) {
                const int i = threadIdx.x * 8 + it * 2048;
                if (i < kc) {
                    put(i, PRO == PRO_RMSNORM ? norm8<A16>(v[it], nwv[it], rstd[t]) : v[it]);
                }
            }
        }
        __syncthreads();
    };

    Unit uA, uB;
    if (nunits > 0) issue(uA, 0);
    if (nunits > 1) issue(uB, 1);
    if (PRO == PRO_RMSNORM) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            if (t >= M) break;
            const bf16_t* xg = a.x + (size_t)t * K;
            float ss = 0.f;
            for (int i = threadIdx.x * 8; i < K; i += 256 * 8) ss = sumsq8<A16>(*reinterpret_cast<const u32x4*>(xg + i), ss);
            ss = block_sum<4>(ss, red);
            rstd[t] = 1.0f / sqrtf(ss / (float)K + a.eps);
        }
    }

    float acc[NR][MT];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[r][t] = 0.f;

    auto consume = [&](const Unit& u, int f) {
        const int bt = f / steps, st = f % steps;
        if (st % spc == 0 && (st > 0 || bt == 0)) stage(st / spc);       // (one chunk: staged once for all the wave's batches)
        const int chunk = st * 64 + lane;
        const bool live = !CH || chunk < nchunks;
        if (live) {
            const int lc = chunk - (st / spc) * (KC / EPL);              // the lane's chunk inside the staged one
            uint32_t op[NR][DOT2 ? NOP : 1];
            float opf[NR][DOT2 ? 1 : NOP];
            float scl[NR], bia[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                scl[r] = SB ? bf16lo(u.sbv[r]) : bf16_to_f32(u.sc[r]);
                bia[r] = SB ? bf16hi(u.sbv[r]) : bf16_to_f32(u.bi[r]);
                if constexpr (CH) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) op[r][i] = field_pair<BITS, A16>(u.wd[r], i);
                } else if constexpr (BITS == 4) {
#pragma unroll
                    for (int wi = 0; wi < W; ++wi) nibble_pairs<A16>(u.wd[r][wi], &op[r][wi * 4]);
                } else {
#pragma unroll
                    for (int wi = 0; wi < W; ++wi)
#pragma unroll
                        for (int b = 0; b < 4; ++b) opf[r][wi * 4 + b] = (float)((u.wd[r][wi] >> (8 * b)) & 0xFFu);
                }
                if (BITS == 4 || CH) bia[r] = fmaf(-A16::kMagic, scl[r], bia[r]);
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                if (t >= M) break;
                uint32_t xp[EPL / 2];
#pragma unroll
                for (int j = 0; j < EPL / 8; ++j) {
                    const u32x4 xv = *reinterpret_cast<const u32x4*>(xs + (size_t)t * KC + (size_t)lc * EPL + j * 8);
#pragma unroll
                    for (int q = 0; q < 4; ++q) xp[j * 4 + q] = xv[q];
                }
                const float xsm = xsum[t * (KC / EPL) + lc];
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    float d = 0.f;
                    if constexpr (DOT2) {
#pragma unroll
                        for (int i = 0; i < NOP; ++i) d = A16::dot2(xp[i], op[r][i], d);
                    } else {
#pragma unroll
                        for (int e = 0; e < NOP; ++e) d = fmaf((e & 1) ? A16::hi(xp[e >> 1]) : A16::lo(xp[e >> 1]), opf[r][e], d);
                    }
                    acc[r][t] = fmaf(scl[r], d, acc[r][t]);
                    acc[r][t] = fmaf(bia[r], xsm, acc[r][t]);
                }
            }
        }
        if (st == steps - 1) {   // the batch's rows are complete: reduce, epilogue, restart the accumulators
            const int r0 = row_base + bt * RB;
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int t = 0; t < MT; ++t)
                    if (t < M) acc[r][t] = wave_sum(acc[r][t]);
            if (lane == 0) {
#pragma unroll
                for (int rr = 0; rr < RB; ++rr) {
                    const int row = r0 + rr;
                    if (row >= N) break;
                    // output element of row t: out [M, N], or member mi's own [M, m[mi].n] (q | k | v into separate buffers)
                    bf16_t* ob = a.out;
                    int col = row, ld = N;
                    if (EPI != EPI_SWIGLU && ra.mout[0]) {
                        int mi = 0;
                        if (col >= a.m[0].n) { col -= a.m[0].n; mi = 1; if (col >= a.m[1].n) { col -= a.m[1].n; mi = 2; } }
                        ob = ra.mout[mi];
                        ld = a.m[mi].n;
                    }
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        if (t >= M) break;
                        const float v0 = acc[LR * rr][t], v1 = acc[LR * rr + (LR - 1)][t];
                        ob[(size_t)t * ld + col] = epi_bits<EPI, A16>(v0, v1, EPI == EPI_RESIDUAL ? a.resid[(size_t)t * N + row] : (bf16_t)0, a.swiglu_single_round);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[r][t] = 0.f;
        }
    };
    for (int f = 0; f < nunits; f += 2) {
        if (f > 0 && f + 1 < nunits) issue(uB, f + 1);
        consume(uA, f);
        if (f + 1 >= nunits) break;
        if (f + 2 < nunits) issue(uA, f + 2);
        consume(uB, f + 1);
    }
}

template <int BITS, int W, int MT>
int launch_rows_w(const QRowsArgs& ra, int pro, int epi, hipStream_t s) {
    constexpr int EPW = 32 / BITS, EPL = quant_chunked(BITS) ? 32 : W * EPW;
    const QGemvArgs& a = ra.g;
    const int KC = a.K <= kc_max(MT) ? a.K : kc_max(MT);
    const size_t shmem = (size_t)MT * KC * 2 + (size_t)MT * (KC / EPL) * 4 + 64;
    const int rb = epi == EPI_SWIGLU ? 2 : 4;
    const dim3 grid((a.N + 4 * rb * ra.nb - 1) / (4 * rb * ra.nb)), block(256);
    bool sb = W == 4 || quant_chunked(BITS);
    for (int i = 0; i < 3 && sb; ++i)
        if (a.m[i].w && !a.m[i].sb) sb = false;
#define OMX_QROWS_LAUNCH(P, E, SBF)                                                                                          \
    {                                                                                                                        \
        const void* fn = (const void*)qgemv_rows_kernel<BITS, W, P, E, MT, SBF>;                                             \
        if (shmem > 64 * 1024) OMX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)); \
        OMX_LAUNCH((qgemv_rows_kernel<BITS, W, P, E, MT, SBF>), grid, block, shmem, s, ra);                                  \
        OMX_LAUNCH_CHECK();                                                                                                  \
        return 0;                                                                                                            \
    }
#define OMX_QROWS_CASE(P, E)                                                 \
    if (pro == P && epi == E) {                                              \
        if constexpr (W == 4 || quant_chunked(BITS)) {                       \
            if (sb) OMX_QROWS_LAUNCH(P, E, true)                             \
        }                                                                    \
        OMX_QROWS_LAUNCH(P, E, false)                                        \
    }
    OMX_QROWS_CASE(PRO_NONE, EPI_STORE)
    OMX_QROWS_CASE(PRO_RMSNORM, EPI_STORE)
    OMX_QROWS_CASE(PRO_NONE, EPI_RESIDUAL)
    OMX_QROWS_CASE(PRO_RMSNORM, EPI_SWIGLU)
    OMX_QROWS_CASE(PRO_NONE, EPI_SWIGLU)
#undef OMX_QROWS_CASE
#undef OMX_QROWS_LAUNCH
    return set_error("quantized rows gemv: unsupported prologue/epilogue combination %d/%d", pro, epi);
}

template <int BITS, int W>
int launch_rows_m(const QRowsArgs& ra, int pro, int epi, hipStream_t s) {
    if (ra.M <= 2) return launch_rows_w<BITS, W, 2>(ra, pro, epi, s);
    if (ra.M <= 4) return launch_rows_w<BITS, W, 4>(ra, pro, epi, s);
    return launch_rows_w<BITS, W, 8>(ra, pro, epi, s);
}

template <int BITS>
int launch_rows_bits(const QRowsArgs& ra_in, int pro, int epi, hipStream_t s) {
    QRowsArgs ra = ra_in;
    const QGemvArgs& a = ra.g;
    constexpr int EPW = 32 / BITS;
    // the single-row kernel's choice of W (quant.hip launch_qgemv_bits): the lane's chunk, and with it the arithmetic, is the same
    int W = 4;
    if constexpr (quant_chunked(BITS)) {
        OMX_REQUIRE(a.K > 0 && a.K % 32 == 0 && a.group >= 32, "quantized rows gemv: K=%d unsupported for %d-bit group %d", a.K, BITS, a.group);
    } else {
        while (W * EPW > 8 && (a.K % (64 * W * EPW) != 0 || W * EPW > a.group)) W >>= 1;
        OMX_REQUIRE(a.K % (64 * W * EPW) == 0 && W * EPW <= a.group && W * EPW >= 8,
                    "quantized rows gemv: K=%d unsupported for %d-bit group %d (K must be a multiple of %d)", a.K, BITS, a.group, 64 * EPW);
    }
    // the vocabulary matrix: 16 rows per wave when K is staged in one chunk (the activation rows staged once per 64 rows, not 16)
    const int kcm = ra.M <= 2 ? kc_max(2) : ra.M <= 4 ? kc_max(4) : kc_max(8);
    ra.nb = (a.N >= 65536 && epi != EPI_SWIGLU && a.K <= kcm) ? 4 : 1;
    if constexpr (quant_chunked(BITS)) {
        return launch_rows_m<BITS, BITS>(ra, pro, epi, s);
    } else {
        if (W == 4) return launch_rows_m<BITS, 4>(ra, pro, epi, s);
        if (W == 2) return launch_rows_m<BITS, 2>(ra, pro, epi, s);
        if constexpr (BITS == 4) return launch_rows_m<BITS, 1>(ra, pro, epi, s);
        return set_error("quantized rows gemv: K=%d too small for %d-bit weights", a.K, BITS);
    }
}

}  // namespace

int launch_qgemv_rows(const QRowsArgs& ra, int bits, int pro, int epi, hipStream_t s) {
    const QGemvArgs& a = ra.g;
    OMX_REQUIRE(ra.M >= 1 && ra.M <= 8, "quantized rows gemv: M=%d (1..8 rows per launch)", ra.M);
    OMX_REQUIRE(a.x && (a.out || (ra.mout[0] && epi != EPI_SWIGLU)) && a.m[0].w && a.m[0].scales && a.N > 0 && a.K > 0, "quantized rows gemv: null tensor or empty shape");
    OMX_REQUIRE(!a.scales_f16 && !a.w_sel && a.w_sel_n == 0 && (a.n_batch <= 1 || a.n_batch == ra.M) && (a.x_div <= 1),
                "quantized rows gemv: bf16 triplets of one dense matrix only");
    OMX_REQUIRE(a.group == 32 || a.group == 64 || a.group == 128, "quantized rows gemv: group %d", a.group);
    OMX_REQUIRE(pro != PRO_RMSNORM || a.norm_w, "quantized rows gemv: RMSNorm prologue without norm weights");
    OMX_REQUIRE(epi != EPI_RESIDUAL || a.resid, "quantized rows gemv: residual epilogue without the residual rows");
    OMX_REQUIRE(epi != EPI_SWIGLU || (a.m[1].w && a.m[0].n == a.N && a.m[1].n == a.N), "quantized rows gemv: SwiGLU needs gate and up of N rows");
    if (epi != EPI_SWIGLU) {
        const int n_stack = a.m[0].n + (a.m[1].w ? a.m[1].n : 0) + (a.m[2].w ? a.m[2].n : 0);
        OMX_REQUIRE(n_stack == a.N, "quantized rows gemv: stacked members hold %d rows, N = %d", n_stack, a.N);
        for (int i = 0; i < 3 && !a.out; ++i) OMX_REQUIRE(!a.m[i].w || ra.mout[i], "quantized rows gemv: no output for member %d", i);
    }
    switch (bits) {
    case 2: return launch_rows_bits<2>(ra, pro, epi, s);
    case 3: return launch_rows_bits<3>(ra, pro, epi, s);
    case 4: return launch_rows_bits<4>(ra, pro, epi, s);
    case 5: return launch_rows_bits<5>(ra, pro, epi, s);
    case 6: return launch_rows_bits<6>(ra, pro, epi, s);
    case 8: return launch_rows_bits<8>(ra, pro, epi, s);
    default: return set_error("quantized rows gemv: bits must be 2, 3, 4, 5, 6 or 8 (got %d)", bits);
    }
}

}  // namespace omx
