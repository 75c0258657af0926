// The text of the packed-weight decode GEMV (quant.hip), included by qgemv_kernel and by qgemv_member: block QGB_BX of a launch over
// QGB_N rows in groups of QGB_GROUP elements, inside a function whose template parameters / constants are BITS, W, PRO, EPI, RB, SB,
// F16S and whose launch arguments are `a`.  qgemv_kernel: the rows of the stack a.m[0 .. 2] (QGB_FIND_MEMBER walks it, QGB_MEMBER =
// a.m[mi], QGB_COL0 empty).  qgemv_member (one member of a mixed-format stack): the rows of the one matrix QGB_MEMBER in ITS format,
// written from column QGB_COL0 of the output row.  Per row the arithmetic is the same, so a matrix's rows do not depend on the launch
// that computes them.  An include, not a function: moved behind a __forceinline__ call the same text changed the register allocation
// of 102 of qgemv_kernel's instantiations (DESIGN 4.9); included, every one of them compiles to what it compiled to before.
    typedef Act16<F16S> A16;                                // activations / outputs: bfloat16, or float16 for a float16 checkpoint (F16S)
    constexpr bool CH = quant_chunked(BITS);
    static_assert(!CH || W == BITS, "a chunked width streams one run of BITS words per lane and step");
    constexpr int EPW = 32 / BITS, EPL = CH ? 32 : W * EPW;          // elements per lane per step
    constexpr int LR = (EPI == EPI_SWIGLU) ? 2 : 1;         // physical rows per logical row
    constexpr int NR = RB * LR;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem);                       // [K]
    float* xsum = reinterpret_cast<float*>(smem + (size_t)a.K * 2);     // [K / EPL]
    float* red = xsum + a.K / EPL;                                      // [8]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int by = blockIdx.y;
    const bf16_t* xg = a.x + (size_t)(by / a.x_div) * a.K;
    size_t e = a.w_sel ? a.w_sel[by] : 0;
    if (!local_expert(e, a.w_sel_lo, a.w_sel_n)) return;      // a slot routed to another rank's expert (block-uniform: before any barrier)
    bf16_t* out = a.out + (size_t)by * a.N QGB_COL0;

    const int steps = CH ? (a.K + 64 * EPL - 1) / (64 * EPL) : a.K / (64 * EPL);
    const int nchunks = a.K / EPL;     // (CH: lanes of the last step at chunk >= nchunks load and add nothing)
    const int words_per_row = CH ? a.K / 32 * BITS : a.K / EPW, groups_per_row = a.K / QGB_GROUP;
    const int row_begin = (QGB_BX * 4 + wave) * a.rows_per_wave;
    const int row_end = min(row_begin + a.rows_per_wave, QGB_N);
    uint64_t best = 0;
    // physical row pr of the batch: which member matrix, which row inside it
    auto locate = [&](int pr, const uint32_t*& wq, const bf16_t*& sc, const bf16_t*& bi, const uint32_t*& sbp) {
        int mi, row;
        if (EPI == EPI_SWIGLU) {
            mi = pr & 1;
            row = min(pr >> 1, QGB_N - 1);
        } else {
            row = min(pr, QGB_N - 1);
            mi = 0;
            QGB_FIND_MEMBER
        }
        const QMat& M = QGB_MEMBER;
        wq = M.w + e * a.w_estride + (size_t)row * words_per_row;
        sc = M.scales + e * a.s_estride + (size_t)row * groups_per_row;
        bi = M.biases ? M.biases + e * a.s_estride + (size_t)row * groups_per_row : nullptr;
        sbp = SB ? M.sb + e * a.s_estride + (size_t)row * groups_per_row : nullptr;
    };
    // A "unit" = one K step of one batch of RB logical rows (NR physical rows): NR x W words + NR scales + NR biases per
    // lane.  Units of consecutive steps / batches are streamed through TWO register sets: the loads of unit f+1 are in
    // flight while unit f is multiplied (the weights are read once, straight to registers, non-temporal).
    struct Unit {
        uint32_t wd[NR][W];
        bf16_t sc[NR], bi[NR];
        uint32_t sbv[NR];
    };
    const int nbatch = (row_end - row_begin + RB - 1) / RB;
    const int nunits = nbatch > 0 ? nbatch * steps : 0;
    const uint32_t* rw[NR];      // row pointers of the batch being ISSUED (issue order is monotonic in f)
    const bf16_t* rs[NR];
    const bf16_t* rb[NR];
    const uint32_t* rsb[NR];
    auto issue = [&](Unit& u, int f) {
        const int st = f % steps;
        if (st == 0) {
            const int r0 = row_begin + (f / steps) * RB;
#pragma unroll
            for (int r = 0; r < NR; ++r) locate(EPI == EPI_SWIGLU ? 2 * (r0 + r / 2) + (r & 1) : r0 + r, rw[r], rs[r], rb[r], rsb[r]);
        }
        const int chunk = st * 64 + lane;
        const int g = chunk * EPL / QGB_GROUP;
        if constexpr (CH) {
            if (chunk >= nchunks) return;    // (never consumed: see consume)
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint32_t* p = rw[r] + (size_t)chunk * W;
            if constexpr (CH) {
                // BITS words at a 4-byte aligned address (the x3 / x4 forms need only dword alignment on gfx950)
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
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
    auto consume = [&](const Unit& u, int f) {
        const int r0 = row_begin + (f / steps) * RB, st = f % steps;
        const int chunk = st * 64 + lane;
        const bool live = !CH || chunk < nchunks;
        uint32_t xp[EPL / 2];   // the lane's activations, still packed bf16 pairs
        if (live) {
#pragma unroll
            for (int j = 0; j < EPL / 8; ++j) {
                const u32x4 xv = *reinterpret_cast<const u32x4*>(xs + (size_t)chunk * EPL + j * 8);
#pragma unroll
                for (int q = 0; q < 4; ++q) xp[j * 4 + q] = xv[q];
            }
            const float xsm = xsum[chunk];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                float d = 0.f;
                const float scl = SB ? (F16S ? scale_to_f32<true>((uint16_t)u.sbv[r]) : bf16lo(u.sbv[r])) : scale_to_f32<F16S>(u.sc[r]);
                float bia = SB ? (F16S ? scale_to_f32<true>((uint16_t)(u.sbv[r] >> 16)) : bf16hi(u.sbv[r])) : scale_to_f32<F16S>(u.bi[r]);
                if constexpr (CH) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) d = A16::dot2(xp[i], A16::unmagic(field_pair<BITS, A16>(u.wd[r], i)), d);
                }
#pragma unroll
                for (int wi = 0; wi < (CH ? 0 : W); ++wi) {
                    const uint32_t wdw = u.wd[r][wi];
                    if (BITS == 4) {
                        uint32_t qp[4];   // (the activations were stored in LDS in the order of these pairs: put() below)
                        nibble_pairs<A16>(wdw, qp);
#pragma unroll
                        for (int k = 0; k < 4; ++k) d = A16::dot2(xp[wi * 4 + k], A16::unmagic(qp[k]), d);
                    } else {
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const uint32_t xw = xp[wi * 2 + (b >> 1)];
                            d = fmaf((b & 1) ? A16::hi(xw) : A16::lo(xw), (float)((wdw >> (8 * b)) & 0xFFu), d);
                        }
                    }
                }
                if (BITS == 4 || CH) bia = fmaf(-A16::kMagic, scl, bia);
                acc[r] = fmaf(scl, d, acc[r]);
                acc[r] = fmaf(bia, xsm, acc[r]);
            }
        }
        if (st == steps - 1) {   // the batch's rows are complete: reduce, epilogue, restart the accumulators
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r] = wave_sum(acc[r]);
            if (lane == 0) {
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const int row = r0 + r;
                    if (row >= row_end) break;
                    const float v0 = acc[LR * r], v1 = acc[LR * r + (LR - 1)];
                    if constexpr (EPI == EPI_F32) {
                        a.out_f32[(size_t)by * a.N QGB_COL0 + row] = v0;
                    } else {
                        const bf16_t lb = epi_bits<EPI, A16>(v0, v1, EPI == EPI_RESIDUAL ? a.resid[row] : (bf16_t)0, a.swiglu_single_round);
                        out[row] = lb;
                        if (EPI == EPI_ARGMAX) {
                            const uint64_t key = argmax_key(A16::val(lb), (uint32_t)(row + a.row_offset));
                            best = key > best ? key : best;
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r] = 0.f;
        }
    };
    // the first two units go out before the activation is even loaded: they depend on the weights only
    Unit uA, uB;
    if (nunits > 0) issue(uA, 0);
    if (nunits > 1) issue(uB, 1);

    // ---- prologue: x -> LDS as bf16 (RMS-normalised on the way in) and, in the same pass, the per-chunk sums
    //      sum(x_i) that every row's bias term shares (EPL elements = EPL/8 consecutive threads, reduced by DPP) ----
    static_assert(EPL >= 8, "a lane chunk must cover at least one 16-byte activation vector");
    auto put = [&](int i, const u32x4 o) { stage_chunk<A16, EPL, BITS == 4>(xs, xsum, i, o); };
    if (PRO == PRO_RMSNORM && a.K <= 4096) {
        // the hidden-sized prologues (q/k/v, gate/up, lm_head: K <= 4096 = two vectors per thread): the row and the norm weights stay in
        // registers between the two passes -- one global round trip instead of two in a launch that is a chain of them.  Same sums.
        u32x4 raw[2], nwv[2];
        float ss = 0.f;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = threadIdx.x * 8 + it * 2048;
            if (i < a.K) {
                raw[it] = *reinterpret_cast<const u32x4*>(xg + i);
                nwv[it] = *reinterpret_cast<const u32x4*>(a.norm_w + i);
            }
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            if (threadIdx.x * 8 + it * 2048 < a.K) ss = sumsq8<A16>(raw[it], ss);
        }
        ss = block_sum<4>(ss, red);
        const float rstd = 1.0f / sqrtf(ss / (float)a.K + a.eps);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = threadIdx.x * 8 + it * 2048;
            if (i < a.K) put(i, norm8<A16>(raw[it], nwv[it], rstd));
        }
    } else if (PRO == PRO_RMSNORM) {
        float ss = 0.f;
        for (int i = threadIdx.x * 8; i < a.K; i += 256 * 8) ss = sumsq8<A16>(*reinterpret_cast<const u32x4*>(xg + i), ss);
        ss = block_sum<4>(ss, red);
        const float rstd = 1.0f / sqrtf(ss / (float)a.K + a.eps);
        for (int i = threadIdx.x * 8; i < a.K; i += 256 * 8) {
            const u32x4 raw = *reinterpret_cast<const u32x4*>(xg + i);
            put(i, norm8<A16>(raw, *reinterpret_cast<const u32x4*>(a.norm_w + i), rstd));
        }
    } else if (a.K <= 8 * 2048 && !a.rolled_stage) {
        // all of the row's vectors of this thread in flight at once (the rolled loop below waits for each 16-byte load before it
        // issues the next: six dependent L2 round trips in the down projection's prologue, K = 12288)
        u32x4 v[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int i = threadIdx.x * 8 + it * 2048;
            if (i < a.K) v[it] = *reinterpret_cast<const u32x4*>(xg + i);
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int i = threadIdx.x * 8 + it * 2048;
            if (i < a.K) put(i, v[it]);
        }
    } else {
        for (int i = threadIdx.x * 8; i < a.K; i += 256 * 8) put(i, *reinterpret_cast<const u32x4*>(xg + i));
    }
    __syncthreads();

    for (int f = 0; f < nunits; f += 2) {
        if (f > 0 && f + 1 < nunits) issue(uB, f + 1);
        consume(uA, f);
        if (f + 1 >= nunits) break;
        if (f + 2 < nunits) issue(uA, f + 2);
        consume(uB, f + 1);
    }
    if (EPI == EPI_ARGMAX) {
        uint64_t* bred = reinterpret_cast<uint64_t*>(red);
        __syncthreads();
        if (lane == 0) bred[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t b = bred[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) b = bred[w] > b ? bred[w] : b;
            a.argmax_slot[QGB_BX] = b;
        }
    }
