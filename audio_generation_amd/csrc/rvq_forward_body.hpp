    // The statements of the RVQ forward kernel: included by rvq.hip, once per kernel, inside
    //     template <int MT, bool TAIL_LDS> __global__ void rvq_forward_kernel(RvqArgs a)                                (STAGED = false)
    //     template <int MT, bool TAIL_LDS> __global__ void rvq_forward_staged_kernel(RvqArgs a, const int64_t *stages)  (STAGED = true)
    // with `a`, `stages` (one int64 stage count per batch row) and the constexpr bool STAGED in scope.  Not a header of its own.
    extern __shared__ __attribute__((aligned(16))) char smem_b[];
    const int Dp = rvq_dp(a.D), RSF = rvq_rsf(Dp), NG = Dp / 8;
    const RvqLds L = rvq_lds_map(Dp, a.K, a.Q, TAIL_LDS);
    float *R = reinterpret_cast<float *>(smem_b + L.R);           // [FT][RSF]
    char *PL = smem_b + L.PL;                                     // [2][NG][PROW]: frame f of group g at g PROW + 16 f
    double *SQ = reinterpret_cast<double *>(smem_b + L.PL);       // [SQ_PAIRS][Dp]  (between the score passes and the update)
    float *wmin = reinterpret_cast<float *>(smem_b + L.wmin);     // [2][NWV][FT]
    float *rn2 = reinterpret_cast<float *>(smem_b + L.rn2);       // [FT]   ||r - mu||^2 of the current stage
    float *sqf = reinterpret_cast<float *>(smem_b + L.sqf);       // [FT]   ||r||^2 after the stage's update
    float *musb = reinterpret_cast<float *>(smem_b + L.mus);      // [2][MP] mean codeword of stage q in buffer q & 1
    int *cnt = reinterpret_cast<int *>(smem_b + L.cnt);           // [FT]
    int *state = reinterpret_cast<int *>(smem_b + L.state);       // [FT] 0 decided / 1 exact among cands / 2 full
    int *best = reinterpret_cast<int *>(smem_b + L.best);         // [FT]
    int *ccode = reinterpret_cast<int *>(smem_b + L.ccode);       // [FT][CAND]
    float *cscore = reinterpret_cast<float *>(smem_b + L.cscore); // [FT][CAND]
    double *cdist = reinterpret_cast<double *>(smem_b + L.cdist); // [FT][CAND]
    int *work = reinterpret_cast<int *>(smem_b + L.work);         // [FT * CAND] (frame, candidate) pairs that need the exact distance
    int *flags = reinterpret_cast<int *>(smem_b + L.flags);       // [0] number of pairs, [1] any frame in candidate overflow
    int *hist = reinterpret_cast<int *>(smem_b + L.hist);         // [Q][FT] the chosen codes (x_q is rebuilt from them)
    float *tailsb = reinterpret_cast<float *>(smem_b + L.tails);  // [2][TP] c2 | cn of stage q in buffer q & 1 (TAIL_LDS)
    const int MP = rvq_pad64(Dp), TP = rvq_pad64(2 * a.K);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t N = int64_t(a.B) * a.T;
    const int64_t n0 = int64_t(blockIdx.x) * FT;
    const int D = a.D, K = a.K;
    constexpr int FPW = FT / NWV;
    // STAGED: the stage counts of this wave's frames (wave-uniform; a padding frame of the last workgroup has none)
    int qf[STAGED ? FPW : 1];
    if constexpr (STAGED) {
#pragma unroll
        for (int j = 0; j < FPW; ++j) {
            const int64_t n = n0 + __builtin_amdgcn_readfirstlane(wave) + j * NWV;
            qf[j] = __builtin_amdgcn_readfirstlane(count_clamp(n < N ? stages[n / a.T] : 0, a.Q));
        }
    }
    auto live_at = [&](int j, int q) {             // is stage q of this wave's frame j live?
        if constexpr (STAGED) return q < qf[j];
        else return true;
    };
    auto stage_end = [&](int j) {                  // the stage bound of this wave's frame j
        if constexpr (STAGED) return qf[j];
        else return a.Q;
    };

    RVQ_STAMP(0, true);
    // ---- stage the latents: R[f][d] = x[n0+f][d] (zero for d >= D and for frames past the end); pick the coalesced order ----
    if (a.x_st == 1 || a.x_sd != 1) {  // time-contiguous ("b c l"): frames fastest
        for (int e = tid; e < RSF * FT; e += NT) {
            const int d = e >> 5, f = e & 31;
            const int64_t n = n0 + f;
            float v = 0.f;
            if (d < D && n < N) {
                const int64_t b = n / a.T, t = n - b * a.T;
                v = a.x[b * a.x_sb + t * a.x_st + d * a.x_sd];
            }
            R[f * RSF + d] = v;
        }
    } else {  // channel-contiguous ("b l c"): d fastest
        for (int f = wave; f < FT; f += NWV) {
            const int64_t n = n0 + f;
            const int64_t b = n < N ? n / a.T : 0, t = n < N ? n - b * a.T : 0;
            const float *src = a.x + b * a.x_sb + t * a.x_st;
            for (int d = lane; d < RSF; d += 64) R[f * RSF + d] = (d < D && n < N) ? src[d] : 0.f;
        }
    }
    // the 8 dims d0 .. d0 + 7 of a codeword row: the LOADS only, from clamped addresses (a select on the loaded value would make
    // the wave wait for each row in turn -- four serial L2 round trips per update phase, measured); the elements past D are
    // zeroed by mask_code8 where the row is used
    auto load_code8 = [&](float (&cv)[8], const float *__restrict__ c, int d0) {
        if ((D & 3) == 0) {
            const f32x4 c0 = *reinterpret_cast<const f32x4 *>(c + (d0 < D ? d0 : 0));
            const f32x4 c1 = *reinterpret_cast<const f32x4 *>(c + (d0 + 4 < D ? d0 + 4 : 0));
#pragma unroll
            for (int e = 0; e < 4; ++e) cv[e] = c0[e], cv[4 + e] = c1[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) cv[e] = c[min(d0 + e, D - 1)];
        }
    };
    auto mask_code8 = [&](float (&cv)[8], int d0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) cv[e] = d0 + e < D ? cv[e] : 0.f;
    };
    // The pass between two stages over a wave's FPW frames (w, w + NWV, ...), lane L on dims d0 = 8 L .. 8 L + 7 (+ 512 per round):
    //   r -= c (c = the chosen codeword; not before stage 0), squared residual, r' = fl(r - mu) with the NEXT stage's mean,
    //   ||r'||^2, and the two bf16 pieces of r' into the planes.  All frames' loads first, then the arithmetic, then the stores:
    //   the frames' latencies overlap instead of adding up.  red[2 j] += sum r^2, red[2 j + 1] += sum r'^2 of frame j (this lane's part).
    auto frames_pass = [&](float (&cv)[FPW][8], bool sub, const float *mus, int d0, float (&red)[2 * FPW]) {
        f32x4 r0[FPW], r1[FPW];
#pragma unroll
        for (int j = 0; j < FPW; ++j) {
            const float *rr = R + (wave + j * NWV) * RSF + d0;
            r0[j] = *reinterpret_cast<const f32x4 *>(rr), r1[j] = *reinterpret_cast<const f32x4 *>(rr + 4);
        }
        f32x4 m0 = {0.f, 0.f, 0.f, 0.f}, m1 = m0;
        if (mus != nullptr) m0 = *reinterpret_cast<const f32x4 *>(mus + d0), m1 = *reinterpret_cast<const f32x4 *>(mus + d0 + 4);
#pragma unroll
        for (int j = 0; j < FPW; ++j) {
            const int f = wave + j * NWV;
            if (sub) {
                mask_code8(cv[j], d0);
#pragma unroll
                for (int e = 0; e < 4; ++e) r0[j][e] -= cv[j][e], r1[j][e] -= cv[j][4 + e];
                float *rr = R + f * RSF + d0;
                *reinterpret_cast<f32x4 *>(rr) = r0[j];
                *reinterpret_cast<f32x4 *>(rr + 4) = r1[j];
            }
            rvq_bf16x8 h8, m8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float rv = e < 4 ? r0[j][e] : r1[j][e - 4];
                red[2 * j] = fmaf(rv, rv, red[2 * j]);
                const float v = rv - (e < 4 ? m0[e] : m1[e - 4]);
                red[2 * j + 1] = fmaf(v, v, red[2 * j + 1]);
                const __bf16 hh = (__bf16)v;
                h8[e] = hh;
                m8[e] = (__bf16)(v - (float)hh);
            }
            if (mus != nullptr) {   // (after the last stage only the squared residual is wanted)
                const int g = d0 >> 3;
                *reinterpret_cast<rvq_bf16x8 *>(PL + g * PROW + f * 16) = h8;
                *reinterpret_cast<rvq_bf16x8 *>(PL + (NG + g) * PROW + f * 16) = m8;
            }
        }
    };
    auto wave_sums = [&](float (&red)[2 * FPW]) {      // the 2 FPW sums over the lanes (uniform results), chains side by side
#pragma unroll
        for (int i = 0; i < 2 * FPW; ++i) red[i] = rvq_wave_sum(red[i]);
    };
    // |c'|^2 | |c'| (adjacent in the image) and the mean codeword of stage qn -> buffer qn & 1, by LDS-DMA (a dword per lane, 256 B
    // per instruction, issued by all waves in turn): no registers are held across the search and nothing is copied afterwards.
    // Lanes past the end re-read the last element into the buffer's padding.
    auto dma_tables = [&](int qn) {
        const float *c2n = a.packed + qn * rvq_stage_floats(K, D) + size_t(Dp) * K;
        const float *mun = c2n + 2 * size_t(K) + 4;
        if (TAIL_LDS)
            for (int i = wave; i * 64 < 2 * K; i += NWV)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(c2n + min(i * 64 + lane, 2 * K - 1)),
                                                 (__attribute__((address_space(3))) void *)(tailsb + (qn & 1) * TP + i * 64), 4, 0, 0);
        for (int i = wave; i * 64 < Dp; i += NWV)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(mun + min(i * 64 + lane, Dp - 1)),
                                             (__attribute__((address_space(3))) void *)(musb + (qn & 1) * MP + i * 64), 4, 0, 0);
    };
    // Error of one computed score s_k = |c'_k|^2 - 2 dot_k against the exact |r - c_k|^2 - |r'|^2, in units of (|r'| + |c'_k|)^2:
    //   * |c'|^2 table and the two centring roundings: (D + 8) 2^-24 x 1.25 (as for the fp32 score GEMM of rounds 1-2);
    //   * the dot product on two bf16 pieces per operand: each piece pair drops <= 2^-16 of its element and the m.m product
    //     (<= 2^-16) is not formed: <= 3 x 2^-16 |r'||c'| in all;
    //   * its accumulation.  v_mfma_f32_32x32x16_bf16 forms c + sum of 16 exact products.  MODEL of the instruction: the 17 addends
    //     are aligned to the largest one and each is TRUNCATED at the 24th bit of that alignment (<= 2^-23 of the largest addend each),
    //     then the sum is rounded once (<= 2^-24 of the result): |error| <= (17 x 2 + 1) 2^-24 (|c| + sum |a_k b_k|) = 35 x 2^-24 (...)
    //     per instruction -- the constant this model PROVES, and the one used (round 3 used 18, i.e. 2.6 x the worst case measured
    //     but not what the model proves).  The model itself is an empirical characterisation of the hardware
    //     (tools/mfma_bf16_err.hip: equal magnitudes, exponents spread over 2^20, heavy cancellation, large accumulators: correctly
    //     rounded when the addends are of similar size, otherwise off by at most 7.0 x 2^-24 (|c| + sum |a_k b_k|) -- 5 x inside the
    //     constant); tests/test_gpu_rvq_adversarial.py feeds the kernel the operand patterns that would break a tighter model and the
    //     knob rvq_verify re-runs the full defining search beside the fast path.  Worst-case linear growth over the
    //     chain of 3 Dp / 16 instructions with |c| <= the sum of all |products| <= (1 + 2^-7) |r'||c'|;
    //   with |r'||c'| <= (|r'| + |c'|)^2 / 4 and the factor 2 of the score: x 1/2.
    // Far above the typical error (which grows like the square root of the chain length); only the candidate selection
    // depends on it -- a wider margin means more frames decided by the defining binary64 distance, never a different index.
    const float acc_err = 35.f * float(3 * Dp / 16 + 1) * 5.9604645e-8f * (1.f + 0.0078125f);
    const float err_unit = float(D + 8) * 5.9604645e-8f * 1.25f + 0.5f * (RVQ_ACC_SCALE(a) * acc_err + 3.f * 1.5258789e-5f);
    constexpr int CHUNK = NWV * 32 * MT;  // codewords scored per pass
    const int n_chunks = (K + CHUNK - 1) / CHUNK;

    for (int q = 0; q < a.Q; ++q) {
        const float *img = a.packed + q * rvq_stage_floats(K, D);
        const float *c2 = img + size_t(Dp) * K;
        const float *cn = c2 + K;
        const float *cbq = a.cb + size_t(q) * K * D;

        if (q == 0) {   // later stages: all of this is prepared by the previous stage's update phase (C)
            if (tid < FT) cnt[tid] = 0;
            if (tid < 2) flags[tid] = 0;
            dma_tables(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            // r' = fl(r - mu), ||r'||^2 and the planes of stage 0 (wave w owns frames w, w + NWV, ...)
            {
                float red[2 * FPW], none[FPW][8];
#pragma unroll
                for (int i = 0; i < 2 * FPW; ++i) red[i] = 0.f;
                for (int d0 = 8 * lane; d0 < Dp; d0 += 512) frames_pass(none, false, musb, d0, red);
                wave_sums(red);
                if (lane == 0) {
#pragma unroll
                    for (int j = 0; j < FPW; ++j) rn2[wave + j * NWV] = red[2 * j + 1];
                }
            }
            __syncthreads();
        }
        // The next stage's tables stream into the other buffers during this stage's search (everyone left them at the barrier
        // that ended stage q - 1's search).
        const bool more = q + 1 < a.Q;
        if (more) dma_tables(q + 1);
        const float *tails = tailsb + (q & 1) * TP;
        // Error bound of one computed score: |s_k + |r'|^2 - |r - c_k|^2| <= E_k = eu (|r'| + |c'_k|)^2
        // (fp32 MFMA chain and |c'|^2: (D+2) u (c'^2 + 2 r'c'); the two centring roundings: 2 u (r'+c')^2).
        // Per CODEWORD, not per codebook: one far-away outlier codeword must not widen the margin of
        // the near ones.  k is a candidate iff its lower bound s_k - E_k does not exceed
        // U = min_j (s_j + E_j), the smallest upper bound -- the true arg-min always qualifies.
        const float rnorm = sqrtf(rn2[li]);
        const float eu = 1.01f * err_unit;
        float running = INFINITY;
        const bool stq = q == a.stamp_q;
        RVQ_STAMP(2, stq);

        for (int ch = 0; ch < n_chunks; ++ch) {
            const int code0 = ch * CHUNK + wave * (32 * MT);
            f32x16 acc[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
            int acol[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) acol[i] = min(code0 + i * 32 + li, K - 1);

            // ---- A: scores on the bf16 matrix pipe.  A[i=code][k=d], B[k=d][j=frame].  Both operands are two bf16 pieces
            // (x = h + m + O(2^-16 x)); a 16-deep block of d is three v_mfma_f32_32x32x16_bf16 per subtile -- m.h, h.m, h.h
            // (small terms first; m.m is below 2^-16 of the product and goes into the error bound) -- 96 cycles against 512
            // for the same block on the fp32-input MFMA.  The scores only SELECT candidates: every decision is still made
            // on the bound below and, among several candidates, by the defining binary64 distance, so the indices
            // do not depend on this arithmetic.  Lane (code, half) holds dims 16 kq + 8 half + (0..7): the codeword pieces
            // are two 16-byte loads of the CbH image straight from L2, requested NB - 1 blocks ahead into a ring of register
            // sets (statically addressed: the loop is unrolled by NB); the residual pieces are two conflict-free
            // ds_read_b128 of the planes, one block ahead.
            const char *pb = PL + lh * PROW + li * 16;
            const char *ab = reinterpret_cast<const char *>(img) + size_t(lh) * K * 16;
            constexpr int NB = 4;
            rvq_bf16x8 a_r[NB][MT][2];
            rvq_bf16x8 bh_cur, bm_cur, bh_nxt, bm_nxt;
            const int nblk = Dp / 16;
            auto load_a = [&](rvq_bf16x8 (&dst)[MT][2], int kq) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl)
                        dst[i][pl] = *reinterpret_cast<const rvq_bf16x8 *>(ab + (size_t(kq * 2 + pl) * 2 * K + acol[i]) * 16);
            };
            auto load_b = [&](rvq_bf16x8 &bh, rvq_bf16x8 &bm, int kq) {
                bh = *reinterpret_cast<const rvq_bf16x8 *>(pb + 2 * kq * PROW);
                bm = *reinterpret_cast<const rvq_bf16x8 *>(pb + (NG + 2 * kq) * PROW);
            };
#pragma unroll
            for (int pb0 = 0; pb0 < NB - 1; ++pb0) load_a(a_r[pb0], pb0 < nblk ? pb0 : 0);
            load_b(bh_cur, bm_cur, 0);
            for (int k0 = 0; k0 < nblk; k0 += NB) {
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int kq = k0 + u;
                    if (kq < nblk) {      // wave-uniform
                        const int kf = kq + NB - 1 < nblk ? kq + NB - 1 : 0;      // past the end the prefetch re-reads block 0
                        const int kn = kq + 1 < nblk ? kq + 1 : 0;
                        load_a(a_r[(u + NB - 1) % NB], kf);
                        load_b(bh_nxt, bm_nxt, kn);
#pragma unroll
                        for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_r[u][i][1], bh_cur, acc[i], 0, 0, 0);
#pragma unroll
                        for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_r[u][i][0], bm_cur, acc[i], 0, 0, 0);
#pragma unroll
                        for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_r[u][i][0], bh_cur, acc[i], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        bh_cur = bh_nxt;
                        bm_cur = bm_nxt;
                    }
                }
            }
            RVQ_STAMP(3 + 3 * min(ch, 1), stq);
            // lower bounds in place; rows of register r: (r&3) + 8*(r>>2) + 4*lh.  One subtile at a
            // time (the sched_barrier keeps hipcc from hoisting all 2*16*MT table loads at once,
            // which spills at 2 waves/SIMD).
            float m = INFINITY;
            if (TAIL_LDS && (K & 3) == 0) {   // the four codes of a register group are consecutive: one 16-byte read per table
#pragma unroll
                for (int i = 0; i < MT; ++i) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int cb0 = code0 + i * 32 + 8 * g + 4 * lh;
                        const int cc = min(cb0, K - 4);
                        const f32x4 t2 = *reinterpret_cast<const f32x4 *>(tails + cc), tn = *reinterpret_cast<const f32x4 *>(tails + K + cc);
#pragma unroll
                        for (int e4 = 0; e4 < 4; ++e4) {
                            const int r = 4 * g + e4;
                            const float s = (cb0 < K) ? (t2[e4] - 2.f * acc[i][r]) : INFINITY;
                            const float rc = rnorm + tn[e4];
                            const float e = eu * rc * rc;
                            acc[i][r] = s - e;          // keep the lower bound
                            m = fminf(m, s + e);        // reduce the upper bound
                        }
                    }
                }
            } else
#pragma unroll
            for (int i = 0; i < MT; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int code = code0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const int cc = min(code, K - 1);
                    const float s = (code < K) ? ((TAIL_LDS ? tails[cc] : c2[cc]) - 2.f * acc[i][r]) : INFINITY;
                    const float rc = rnorm + (TAIL_LDS ? tails[K + cc] : cn[cc]);
                    const float e = eu * rc * rc;
                    acc[i][r] = s - e;          // keep the lower bound
                    m = fminf(m, s + e);        // reduce the upper bound
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            m = fminf(m, __shfl_xor(m, 32));
            // (one buffer per pass parity: a wave may post pass ch + 1's minima while another still reads pass ch's -- the only
            // barrier of a pass is the one below)
            float *wm = wmin + (ch & 1) * (NWV * FT);
            if (lh == 0) wm[wave * FT + li] = m;
            __syncthreads();
            RVQ_STAMP(4 + 3 * min(ch, 1), stq);
            float cm = wm[li];
#pragma unroll
            for (int w = 1; w < NWV; ++w) cm = fminf(cm, wm[w * FT + li]);
            running = fminf(running, cm);
            const float thr = running;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float s = acc[i][r];
                    if (s <= thr) {
                        const int code = code0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const int slot = atomicAdd(&cnt[li], 1);
                        if (slot < CAND) {
                            ccode[li * CAND + slot] = code;
                            cscore[li * CAND + slot] = s;
                        }
                    }
                }
            RVQ_STAMP(5 + 3 * min(ch, 1), stq);
        }
        __syncthreads();
        // ---- B: decide ----
        if (tid < FT) {  // wave 0, lane == li == frame
            const int f = tid;
            const int n = cnt[f];
            if (n0 + f >= N) {          // padding frame of the last workgroup (its residual is not a latent): nothing to decide
                best[f] = 0;
                state[f] = 0;
                cnt[f] = 0;
            } else if (n > CAND) {
                state[f] = 2;
                flags[1] = 1;
            } else {
                const float thr = running;
                int kept = 0;
                for (int c = 0; c < n; ++c) {
                    const float s = cscore[f * CAND + c];
                    const int code = ccode[f * CAND + c];
                    if (s <= thr) {
                        ccode[f * CAND + kept] = code;
                        ++kept;
                    }
                }
                cnt[f] = kept;
                if (kept == 0) {  // only reachable with NaN scores: stay in bounds
                    best[f] = 0;
                    state[f] = 0;
                } else if (kept == 1) {
                    best[f] = ccode[f * CAND];
                    state[f] = 0;
                } else {
                    state[f] = 1;
                    const int slot = atomicAdd(&flags[0], kept);
                    for (int c = 0; c < kept; ++c) work[slot + c] = f * CAND + c;
                }
            }
        }
        __syncthreads();
        RVQ_STAMP(9, stq);
        if (a.stamps != nullptr && tid == 0 && stq) a.stamps[size_t(blockIdx.x) * 16 + 14] = (unsigned long long)flags[0];
        // The update phase (C) needs the chosen codeword rows: those of the frames decided by the bounds alone are requested NOW,
        // an L2 round trip (~4 k cycles with every other CU streaming codebooks) that then hides behind the binary64 phase.
        // (before that: this wave's pieces of the next stage's tables, DMA'd at the start of the stage, have long landed -- the wait
        // is free here, and the pick barrier below then publishes them without waiting for the loads issued now)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        float cv[FPW][8];
        bool early[FPW];
#pragma unroll
        for (int j = 0; j < FPW; ++j) {
            const int f = wave + j * NWV;
            early[j] = state[f] == 0;                  // (wave-uniform)
            if (early[j]) load_code8(cv[j], cbq + size_t(best[f]) * D, 8 * lane);
        }
        // The listed (frame, candidate) pairs, SQ_PAIRS at a time: every wave forms the squares of its pairs with all lanes
        // (coalesced codeword loads) into the plane region, then ONE lane per pair adds them in d order -- the pairs' 512-long
        // dependent chains run side by side (lane p / 8 of wave p % 8) instead of one after the other.
        {
            const int n_pairs = flags[0];
            for (int base = 0; base < n_pairs; base += SQ_PAIRS) {   // (uniform)
                const int np = min(SQ_PAIRS, n_pairs - base);
                for (int pp = wave; pp < np; pp += NWV) {
                    const int fc = work[base + pp], f = fc >> 3;
                    rvq_pair_squares(SQ + size_t(pp) * Dp, R + f * RSF, cbq + size_t(ccode[fc]) * D, D, Dp, lane);
                }
                __syncthreads();
                const int pp = lane * NWV + wave;
                if (lane < SQ_PAIRS / NWV && pp < np) cdist[work[base + pp]] = rvq_chain_sum(SQ + size_t(pp) * Dp, D);
                __syncthreads();
            }
        }
        RVQ_STAMP(10, stq);
        if (tid < FT && state[tid] == 1) {
            const int f = tid;
            double bd = cdist[f * CAND];
            int bc = ccode[f * CAND];
            for (int c = 1; c < cnt[f]; ++c) {
                const double dc = cdist[f * CAND + c];
                const int code = ccode[f * CAND + c];
                if (dc < bd || (dc == bd && code < bc)) {
                    bd = dc;
                    bc = code;
                }
            }
            best[f] = bc;
        }
        __syncthreads();
        RVQ_STAMP(11, stq);
        int diag_mx = 0;
        if (RVQ_DIAG(a) && tid == 0)     // DIAGNOSTIC, probe build only (knob b3_dbg = 9): the stage's "squared error" output = largest candidate count
            for (int f = 0; f < FT; ++f) diag_mx = max(diag_mx, state[f] == 2 ? 1000 + cnt[f] : cnt[f]);
        // candidate overflow (degenerate codebooks): full defining search, whole block per frame
        const int any_overflow = flags[1];
        const int kq_bits = __float_as_int(c2[2 * size_t(K) + 1]);
        const int Kq = kq_bits > 0 && kq_bits <= K ? kq_bits : K;     // this stage's codewords (rest of the K rows: padding)
        for (int f = 0; f < (any_overflow ? FT : 0); ++f) {
            if (state[f] != 2) continue;  // uniform across the block (LDS value)
            double bd = INFINITY;
            int bc = 0x7fffffff;
            for (int base = wave * 64; base < Kq; base += NWV * 64) {      // a codeword per lane (rvq_dist_lane)
                const int code = base + lane;
                const double dc = rvq_dist_lane(R + f * RSF, cbq + size_t(min(code, Kq - 1)) * D, D);
                if (code < Kq && (dc < bd || (dc == bd && code < bc))) {
                    bd = dc;
                    bc = code;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {                        // the wave's minimum, lowest index on ties
                const double od = __shfl_xor(bd, off);
                const int oc = __shfl_xor(bc, off);
                if (od < bd || (od == bd && oc < bc)) {
                    bd = od;
                    bc = oc;
                }
            }
            __syncthreads();  // cdist / ccode row 0 are free to reuse as exchange
            if (lane == 0) {
                cdist[wave] = bd;
                ccode[wave] = bc;
            }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < NWV; ++w)
                    if (cdist[w] < bd || (cdist[w] == bd && ccode[w] < bc)) {
                        bd = cdist[w];
                        bc = ccode[w];
                    }
                best[f] = bc;
            }
            __syncthreads();
        }
        RVQ_STAMP(12, stq);
        // ---- C: r -= c, index, squared residual; the next stage's r' = fl(r - mu), its norm and its planes ----
        {
            float red[2 * FPW];
#pragma unroll
            for (int i = 0; i < 2 * FPW; ++i) red[i] = 0.f;
            for (int db = 0; db < Dp; db += 512) {
                const int d0 = db + 8 * lane;
#pragma unroll
                for (int j = 0; j < FPW; ++j)
                    if (db > 0 || !early[j]) load_code8(cv[j], cbq + size_t(best[wave + j * NWV]) * D, d0);
                if (d0 < Dp) frames_pass(cv, true, more ? musb + ((q + 1) & 1) * MP : nullptr, d0, red);
            }
            wave_sums(red);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < FPW; ++j) {
                    const int f = wave + j * NWV;
                    sqf[f] = live_at(j, q) ? red[2 * j] : 0.f;       // the squared residual of this frame (none at a dead stage)
                    rn2[f] = red[2 * j + 1];
                    cnt[f] = 0;                // (read last by the pick step, before the barrier above)
                    hist[q * FT + f] = best[f];
                    if (n0 + f < N) a.index[(n0 + f) * a.Q + q] = live_at(j, q) ? best[f] : -1;
                }
            }
            if (tid == 0) flags[0] = 0;        // (read last at the start of the binary64 phase)
        }
        __syncthreads();                       // the ONE barrier between the update and the next stage's search
        if (tid == 0) {
            flags[1] = 0;                      // (everyone read it right after the pick barrier)
            if (RVQ_DIAG(a)) {
                sqf[0] = float(diag_mx);
                for (int f = 1; f < FT; ++f) sqf[f] = 0.f;
            }
        }
        if (wave == 0) {                  // the stage's squared error: 32 frames, pairwise in double
            double s = (lane < FT && n0 + lane < N) ? double(sqf[lane]) : 0.0;
            for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) a.part[size_t(blockIdx.x) * a.Q + q] = s;   // reduced in a fixed order by rvq_sqerr_kernel
        }
        RVQ_STAMP(13, stq);
    }
    RVQ_STAMP(1, true);
    // ---- x_q = ((0 + c_0) + c_1) + ... rebuilt from the chosen codewords, stage order ----
    const bool q_rows = !(a.q_st == 1 || a.q_sd != 1);     // channel-contiguous output: a frame's row goes out as it is formed
    float *Ot = reinterpret_cast<float *>(smem_b);         // [Dp][RS] transposition tile over R / the planes (both dead now)
    __syncthreads();
    for (int db = 0; db < Dp; db += 512) {
        const int d0 = db + 8 * lane;
#pragma unroll
        for (int j = 0; j < FPW; ++j) {
            const int f = wave + j * NWV;
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = 0.f;
            for (int q0 = 0; q0 < stage_end(j); q0 += 4) { // four stages' rows in flight
                float cv[4][8];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = min(q0 + u, stage_end(j) - 1);
                    load_code8(cv[u], a.cb + (size_t(q) * K + hist[q * FT + f]) * D, d0 < Dp ? d0 : 0);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (q0 + u < stage_end(j)) {
                        mask_code8(cv[u], d0);
#pragma unroll
                        for (int e = 0; e < 8; ++e) o[e] = o[e] + cv[u][e];
                    }
            }
            if (d0 < Dp) {
                if (q_rows) {
                    const int64_t n = n0 + f;
                    if (n < N) {
                        const int64_t b = n / a.T, t = n - b * a.T;
                        float *dst = a.xq + b * a.q_sb + t * a.q_st;
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (d0 + e < D) dst[d0 + e] = o[e];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) Ot[(d0 + e) * RS + f] = o[e];
                }
            }
        }
    }
    if (!q_rows) {
        __syncthreads();
        for (int e = tid; e < D * FT; e += NT) {
            const int d = e >> 5, f = e & 31;
            const int64_t n = n0 + f;
            if (n < N) {
                const int64_t b = n / a.T, t = n - b * a.T;
                a.xq[b * a.q_sb + t * a.q_st + d * a.q_sd] = Ot[d * RS + f];
            }
        }
    }
    RVQ_STAMP(15, true);
