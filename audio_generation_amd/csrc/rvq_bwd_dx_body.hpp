    // The statements of the quantiser backward's dx kernel: included by rvq.hip, once per kernel, inside
    //     template <int QMAX> __global__ void rvq_bwd_dx_kernel(RvqBwdArgs a)                                (STAGED = false)
    //     template <int QMAX> __global__ void rvq_bwd_dx_staged_kernel(RvqBwdArgs a, const int64_t *stages)  (STAGED = true)
    // with `a`, `stages` (one int64 stage count per batch row) and the constexpr bool STAGED in scope.  Not a header of its own.
    __shared__ float xs[BW_TF * BW_RS], gs[BW_TF * BW_RS];
    __shared__ int64_t off[3][BW_TF];
    __shared__ int qfs[STAGED ? BW_TF : 1];             // STAGED: the frames' stage bounds q_f
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * BW_TF, d0 = blockIdx.y * BW_TD;
    const int nf = min(BW_TF, a.n - n0), nd = min(BW_TD, a.dim - d0);
    if (tid < nf) {
        const int n = n0 + tid, b = n / a.t, t = n - b * a.t;
        off[0][tid] = b * a.x_sb + t * a.x_st;
        off[1][tid] = b * a.g_sb + t * a.g_st;
        off[2][tid] = b * a.d_sb + t * a.d_st;
        if constexpr (STAGED) qfs[tid] = count_clamp(stages[b], a.Q);
    }
    __syncthreads();
    auto stage = [&](const float *__restrict__ p, int64_t sd, const int64_t *o, float *tile) {
        if (sd == 1) {
            if (lane < nd)
                for (int f = wave; f < nf; f += 4) tile[f * BW_RS + lane] = p[o[f] + (d0 + lane)];
        } else if (lane < nf) {
            for (int d = wave; d < nd; d += 4) tile[lane * BW_RS + d] = p[o[lane] + (d0 + d) * sd];
        }
    };
    stage(a.x, a.x_sd, off[0], xs);
    if (a.g) stage(a.g, a.g_sd, off[1], gs);
    __syncthreads();
    const float av = (a.g_commit && a.Q > 0) ? *a.g_commit * a.scale : 0.f;
    if (lane < nd) {
        const int d = d0 + lane;
        for (int f = wave; f < nf; f += 4) {
            const int64_t n = n0 + f;
            const int64_t *ix = a.index + n * a.Q;
            int QF = a.Q;                                    // the stage bound of this frame
            if constexpr (STAGED) QF = qfs[f];
            float r = xs[f * BW_RS + lane], rq[QMAX];
#pragma unroll
            for (int q = 0; q < QMAX; ++q) {
                if (q < QF) {
                    const int64_t c = ix[q];
                    if (c >= 0 && c < a.K) r -= a.cb[(int64_t(q) * a.K + c) * a.dim + d];
                }
                rq[q] = r;
            }
            float s = 0.f;
#pragma unroll
            for (int q = QMAX - 1; q >= 0; --q) {
                if (q < QF) {
                    s += rq[q];        // S_{Q-1} = 0 + r_Q
                    if (a.S) a.S[(int64_t(q) * a.n + n) * a.dim + d] = s;
                }
            }
            xs[f * BW_RS + lane] = (a.g ? gs[f * BW_RS + lane] : 0.f) + av * s;
        }
    }
    __syncthreads();
    if (a.d_sd == 1) {
        if (lane < nd)
            for (int f = wave; f < nf; f += 4) a.dx[off[2][f] + (d0 + lane)] = xs[f * BW_RS + lane];
    } else if (lane < nf) {
        for (int d = wave; d < nd; d += 4) a.dx[off[2][lane] + (d0 + d) * a.d_sd] = xs[lane * BW_RS + d];
    }
