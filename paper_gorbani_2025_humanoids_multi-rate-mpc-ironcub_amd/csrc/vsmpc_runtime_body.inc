// Body of the runtime-sized kernels (vsmpc_runtime.hip), included inside solve_kernel_rt (SENS = false) and
// sens_kernel_rt (SENS = true): each kernel declares `constexpr bool SENS` and the pointers cfg, d, in, ws, xout, fmout,
// status_out, iters_out, dxout, dfmout, active_out, flags_out before it.  A textual body (not an inlined device function)
// keeps solve_kernel_rt's code object instruction for instruction what it was before sens_kernel_rt existed.
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const RtSmem s = rt_smem(d, smem);
    const int tid = threadIdx.x, inst = blockIdx.x;
    double* __restrict__ M = ws + size_t(inst) * size_t(d.ws_doubles);
    const int NP = d.np, NZ = d.nz, NU = d.nu, NV = d.nv;

    // ---- P0: record, configuration, linearisation
    for (int i = tid; i < d.nin; i += RT_BLOCK) s.in[i] = in[size_t(inst) * d.nin + i];
    if (tid < d.n) s.dt[tid] = cfg.dt[tid];
    if (tid >= 64 && tid < 64 + NWROWS) s.sq[tid - 64] = cfg.sq[tid - 64];
    if (tid == 0) { s.flags[F_STATUS] = VSMPC_STATUS_MAX_ITER; s.flags[F_ITERS] = 0; }
    __syncthreads();
    double* sA = s.lin;
    double* sBj = sA + NX * NX;
    double* sBt = sBj + NX * NJ;
    double* sC = sBt + NX * NTH;
    p0_linearize<RtTag>(cfg.use_jet, s.in, sA, sBj, sBt, sC, s.vprev, tid, RT_BLOCK);

    // ---- P1: sensitivity recursion of every condensed column, C = sum_k Y_k^T Y_k
    {
        double X[RT_CPT][NX];
        const double* src[RT_CPT];
        int stride[RT_CPT], kind[RT_CPT], blk[RT_CPT];   // kind: 0 joint, 1 throttle, 2 affine, 3 none, 4 parameter
#pragma unroll
        for (int u = 0; u < RT_CPT; ++u) {
            const int c = tid + u * RT_BLOCK;
            kind[u] = c < NU ? 0 : (c < NZ ? 1 : (c == NZ ? 2 : ((SENS && c < NP) ? 4 : 3)));
            blk[u] = kind[u] == 0 ? c >> 3 : (kind[u] == 1 ? (c - NU) >> 2 : 0);
            src[u] = kind[u] == 0 ? sBj + (c & 7) : (kind[u] == 1 ? sBt + ((c - NU) & 3) : sC);
            stride[u] = kind[u] == 0 ? NJ : (kind[u] == 1 ? NTH : 1);
#pragma unroll
            for (int r = 0; r < NX; ++r) X[u][r] = kind[u] == 2 ? s.in[VSMPC_IN_X0 + r] : 0.0;
            if constexpr (SENS) {
#pragma unroll
                for (int r = 0; r < NX; ++r)
                    if (kind[u] == 4 && r == c - NZ - 1) X[u][r] = 1.0;   // parameter column NZ + 1 + i: X_0 = e_i
            }
        }
        double* Y = s.big;   // Y[w * NP + c]
        for (int k = 0; k < d.n; ++k) {
            const double dt = s.dt[k];
            const int jb = rt_joint_block(d, k), tb = rt_throttle_block(d, k);
            const int i = k + 1;                                        // node of X_{k+1}
            const int col = (i - 1) < d.ns ? 0 : (i - 1) - d.ns;      // reference window column (costsVSMPC.cpp:191-200)
#pragma unroll
            for (int u = 0; u < RT_CPT; ++u) {
                if (kind[u] == 3) continue;
                const bool on = kind[u] == 2 || (kind[u] == 0 && blk[u] == jb) || (kind[u] == 1 && blk[u] == tb);
                double nx[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    double a = on ? src[u][r * stride[u]] : 0.0;
#pragma unroll
                    for (int q = 0; q < NX; ++q)
                        if (a_nz(r, q)) a = fma(sA[r * NX + q], X[u][q], a);
                    nx[r] = fma(dt, a, X[u][r]);
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) X[u][r] = nx[r];
                const int c = tid + u * RT_BLOCK;
#pragma unroll
                for (int w = 0; w < NWROWS; ++w) {
                    const int r = wrow(w);
                    const double ref = (kind[u] == 2 && r < 12) ? s.in[VSMPC_IN_XREF + col * 12 + r] : 0.0;
                    Y[w * NP + c] = s.sq[w] * (X[u][r] - ref);
                }
            }
            __syncthreads();
            int ei = 0, ej = 0;
            tri_advance(ei, ej, tid);
            for (size_t e = tid; e < size_t(d.ntri); e += RT_BLOCK) {
                double acc = 0.0;
#pragma unroll
                for (int w = 0; w < NWROWS; ++w) acc = fma(Y[w * NP + ei], Y[w * NP + ej], acc);
                M[e] = k == 0 ? acc : M[e] + acc;
                tri_advance(ei, ej, RT_BLOCK);
            }
            __syncthreads();
        }
    }

    // ---- P2: input costs (every entry touched by exactly one thread), max |gradient| for the release tolerance
    {
        const double w_thr = cfg.w_thr;
        for (int c = tid; c < NZ; c += RT_BLOCK) {
            if (c < NU) {
                const int j = c & 7;
                M[tri(c) + c] += cfg.wj[j];                                   // costsVSMPC.cpp:375-381,564-571
                M[tri(NZ) + c] += cfg.w_reg * s.in[VSMPC_IN_QERR + j];        // :574-589
            } else {
                const int q = c - NU, b = q >> 2, r = q & 3;
                const int npairs = (b < d.nvb - 1 ? 1 : 0) + (b > 0 ? 1 : 0);  // first differences (:383-409)
                double diag = M[tri(c) + c];
                for (int p = 0; p < npairs; ++p) diag += w_thr;
                if (b == 0) diag += cfg.w_init;                                // ThrottleInitialValueCost (:468-487)
                M[tri(c) + c] = diag;
                if (b > 0) M[tri(c) + c - 4] -= w_thr;
                if (b == 0) M[tri(NZ) + c] += -cfg.w_init * s.vprev[r];
            }
        }
        __syncthreads();
        double gm = 0.0;
        for (int c = tid; c < NZ; c += RT_BLOCK) gm = fmax(gm, fabs(M[tri(NZ) + c]));
        s.red[tid] = gm;
        __syncthreads();
        for (int h = RT_BLOCK / 2; h > 0; h >>= 1) {
            if (tid < h) s.red[tid] = fmax(s.red[tid], s.red[tid + h]);
            __syncthreads();
        }
    }
    const double gtol = 1e-10 * (1.0 + s.red[0]);

    // ---- P3: Cholesky of the joint columns; the trailing block becomes (S, s)
    bool bad = false;
    for (int j = 0; j < NU; ++j) {
        const double piv = M[tri(j) + j];
        if (!(piv > 0.0)) { bad = true; break; }   // (every thread reads the same value: a uniform exit)
        const double l = sqrt(piv), il = 1.0 / l;
        for (int i = j + 1 + tid; i < NP; i += RT_BLOCK) {
            const double v = M[tri(i) + j] * il;
            M[tri(i) + j] = v;
            s.col[i] = v;
        }
        __syncthreads();
        if (tid == 0) M[tri(j) + j] = l;           // (after the barrier: every thread has read the pivot)
        const int m = NP - 1 - j;                  // trailing rows / columns j + 1 .. NP - 1
        const size_t nt = size_t(m) * (m + 1) / 2;
        int ei = 0, ej = 0;
        tri_advance(ei, ej, tid);
        for (size_t e = tid; e < nt; e += RT_BLOCK) {
            const int gi = j + 1 + ei, gj = j + 1 + ej;
            M[tri(gi) + gj] -= s.col[gi] * s.col[gj];
            tri_advance(ei, ej, RT_BLOCK);
        }
        __syncthreads();
    }
    const bool factored = !bad;   // the box QP runs (s.state is set)

    // ---- P4: box QP on the throttles, block principal pivoting (executable model: tests/runtime_model.py box_qp)
    const bool hold = s.in[VSMPC_IN_HOLD] != 0.0;
    const double vmin = cfg.vmin, vmax = cfg.vmax;
    double* z = s.z;              // z[0..NU) joints, z[NU..NZ) throttles
    double* zv = z + NU;
    double* sS = M + tri(NZ) + NU;  // reduced gradient s
    if (!bad) {
        for (int p = tid; p < NV; p += RT_BLOCK) s.state[p] = (hold && p < NTH) ? -1 : 0;  // the hold pins v0 at v_prev
        if (tid == 0) { s.flags[F_BEST] = NV + 1; s.flags[F_PATIENCE] = AS_PATIENCE_RT; }
        __syncthreads();
        for (int it = 0; it < cfg.max_as_iter; ++it) {
            // bound values, free list
            for (int p = tid; p < NV; p += RT_BLOCK) {
                const bool fixed = hold && p < NTH;
                const int st = s.state[p];
                if (st != 0) zv[p] = fixed ? s.vprev[p] : (st < 0 ? vmin : vmax);
            }
            if (tid == 0) {
                int nf = 0;
                for (int p = 0; p < NV; ++p)
                    if (s.state[p] == 0) s.idx[nf++] = p;
                s.flags[F_NF] = nf;
            }
            __syncthreads();
            const int nf = s.flags[F_NF];
            double* K = s.big;
            double* rhs = s.vec0;
            double* y = s.vec1;
            // rhs_F = -(s_F + S_FB z_B); K = S_FF (packed lower)
            for (int a = tid; a < nf; a += RT_BLOCK) {
                const int p = s.idx[a];
                double acc = sS[p];
                for (int q = 0; q < NV; ++q)
                    if (s.state[q] != 0) acc = fma(rt_S(M, NU, p, q), zv[q], acc);
                rhs[a] = -acc;
            }
            {
                const size_t nk = size_t(nf) * (nf + 1) / 2;
                int ei = 0, ej = 0;
                tri_advance(ei, ej, tid);
                for (size_t e = tid; e < nk; e += RT_BLOCK) {
                    K[e] = rt_S(M, NU, s.idx[ei], s.idx[ej]);
                    tri_advance(ei, ej, RT_BLOCK);
                }
            }
            __syncthreads();
            // Cholesky of K
            for (int j = 0; j < nf; ++j) {
                const double piv = K[tri(j) + j];
                if (!(piv > 0.0)) { bad = true; break; }
                const double l = sqrt(piv), il = 1.0 / l;
                __syncthreads();   // everyone has read the pivot before it is overwritten
                for (int i = j + 1 + tid; i < nf; i += RT_BLOCK) K[tri(i) + j] *= il;
                if (tid == 0) K[tri(j) + j] = l;
                __syncthreads();
                const int m = nf - 1 - j;
                const size_t nt = size_t(m) * (m + 1) / 2;
                int ei = 0, ej = 0;
                tri_advance(ei, ej, tid);
                for (size_t e = tid; e < nt; e += RT_BLOCK) {
                    const int gi = j + 1 + ei, gj = j + 1 + ej;
                    K[tri(gi) + gj] -= K[tri(gi) + j] * K[tri(gj) + j];
                    tri_advance(ei, ej, RT_BLOCK);
                }
                __syncthreads();
            }
            if (bad) break;
            // L y = rhs, then L^T v = y (v into y)
            for (int j = 0; j < nf; ++j) {
                const double yj = rhs[j] / K[tri(j) + j];
                for (int i = j + 1 + tid; i < nf; i += RT_BLOCK) rhs[i] = fma(-K[tri(i) + j], yj, rhs[i]);
                if (tid == 0) y[j] = yj;
                __syncthreads();
            }
            for (int j = nf - 1; j >= 0; --j) {
                const double vj = y[j] / K[tri(j) + j];
                for (int i = tid; i < j; i += RT_BLOCK) y[i] = fma(-K[tri(j) + i], vj, y[i]);
                __syncthreads();
                if (tid == 0) zv[s.idx[j]] = vj;
            }
            __syncthreads();
            // gradient of the reduced problem at z
            double* grad = s.vec2;
            for (int p = tid; p < NV; p += RT_BLOCK) {
                double acc = sS[p];
                for (int q = 0; q < NV; ++q) acc = fma(rt_S(M, NU, p, q), zv[q], acc);
                grad[p] = acc;
            }
            __syncthreads();
            if (tid == 0) {
                int ninf = 0, last = -1;
                for (int p = 0; p < NV; ++p) {
                    const bool fixed = hold && p < NTH;
                    const int st = s.state[p];
                    const double tol = 1e-12 * (1.0 + fabs(zv[p]));
                    const bool vlo = st == 0 && zv[p] < vmin - tol;
                    const bool vhi = st == 0 && zv[p] > vmax + tol;
                    const bool rel = !fixed && ((st == -1 && grad[p] < -gtol) || (st == 1 && grad[p] > gtol));
                    if (vlo || vhi || rel) { ++ninf; last = p; }
                }
                s.flags[F_ITERS] = it + 1;
                if (ninf == 0) {
                    s.flags[F_STATUS] = VSMPC_STATUS_SOLVED;
                } else {
                    bool all = true;
                    if (ninf < s.flags[F_BEST]) { s.flags[F_BEST] = ninf; s.flags[F_PATIENCE] = AS_PATIENCE_RT; }
                    else if (s.flags[F_PATIENCE] > 0) { --s.flags[F_PATIENCE]; }
                    else all = false;   // single pivot on the largest infeasible index
                    for (int p = 0; p < NV; ++p) {
                        if (!all && p != last) continue;
                        const bool fixed = hold && p < NTH;
                        const int st = s.state[p];
                        const double tol = 1e-12 * (1.0 + fabs(zv[p]));
                        if (st == 0 && zv[p] < vmin - tol) s.state[p] = -1;
                        else if (st == 0 && zv[p] > vmax + tol) s.state[p] = 1;
                        else if (!fixed && ((st == -1 && grad[p] < -gtol) || (st == 1 && grad[p] > gtol))) s.state[p] = 0;
                    }
                }
            }
            __syncthreads();
            if (s.flags[F_STATUS] == VSMPC_STATUS_SOLVED) break;
        }
        __syncthreads();
        // the final point: bound throttles exactly on their bound
        for (int p = tid; p < NV; p += RT_BLOCK) {
            const bool fixed = hold && p < NTH;
            const int st = s.state[p];
            if (st != 0) zv[p] = fixed ? s.vprev[p] : (st < 0 ? vmin : vmax);
        }
        __syncthreads();
    }

    // ---- P4 (SENS): S_FF dv_F = -F~_F for the 26 parameter rows, in place (row j's throttle entry p at
    // M[tri(NZ + 1 + j) + NU + p]); the last iteration's factor of S_FF is still in K
    const bool sens_ok = SENS && !bad && s.flags[F_STATUS] == VSMPC_STATUS_SOLVED;
    if constexpr (SENS) {
        if (sens_ok) {
            const int nf = s.flags[F_NF];
            const double* K = s.big;
            const int* idx = s.idx;
            for (int e = tid; e < NV * RT_NPAR; e += RT_BLOCK) {
                const int p = e / RT_NPAR, j = e % RT_NPAR;
                double* r = M + tri(NZ + 1 + j) + NU + p;
                *r = s.state[p] == 0 ? -*r : 0.0;     // bounds and the hold pin do not depend on X0
            }
            __syncthreads();
            for (int a = 0; a < nf; ++a) {            // L y = rhs
                if (tid < RT_NPAR) M[tri(NZ + 1 + tid) + NU + idx[a]] /= K[tri(a) + a];
                __syncthreads();
                for (int e = tid; e < (nf - 1 - a) * RT_NPAR; e += RT_BLOCK) {
                    const int i = a + 1 + e / RT_NPAR, j = e % RT_NPAR;
                    double* row = M + tri(NZ + 1 + j) + NU;
                    row[idx[i]] = fma(-K[tri(i) + a], row[idx[a]], row[idx[i]]);
                }
                __syncthreads();
            }
            for (int a = nf - 1; a >= 0; --a) {       // L^T dv = y
                if (tid < RT_NPAR) M[tri(NZ + 1 + tid) + NU + idx[a]] /= K[tri(a) + a];
                __syncthreads();
                for (int e = tid; e < a * RT_NPAR; e += RT_BLOCK) {
                    const int i = e / RT_NPAR, j = e % RT_NPAR;
                    double* row = M + tri(NZ + 1 + j) + NU;
                    row[idx[i]] = fma(-K[tri(a) + i], row[idx[a]], row[idx[i]]);
                }
                __syncthreads();
            }
        }
    }

    // ---- P5: joints, L_jj^T u = -(L_vj^T v + l_j)
    if (!bad) {
        double* r = s.col;
        for (int j = tid; j < NU; j += RT_BLOCK) {
            double acc = M[tri(NZ) + j];
            for (int p = 0; p < NV; ++p) acc = fma(M[tri(NU + p) + j], zv[p], acc);
            r[j] = -acc;
        }
        __syncthreads();
        for (int j = NU - 1; j >= 0; --j) {
            const double uj = r[j] / M[tri(j) + j];
            for (int i = tid; i < j; i += RT_BLOCK) r[i] = fma(-M[tri(j) + i], uj, r[i]);
            __syncthreads();
            if (tid == 0) z[j] = uj;
        }
        __syncthreads();
    }

    // ---- P5 (SENS): L_jj^T du = -(L_vj^T dv + l~), in place in the joint entries of the parameter rows
    if constexpr (SENS) {
        if (sens_ok) {
            for (int e = tid; e < NU * RT_NPAR; e += RT_BLOCK) {
                const int jj = e / RT_NPAR, j = e % RT_NPAR;
                double* row = M + tri(NZ + 1 + j);
                double acc = row[jj];
                for (int p = 0; p < NV; ++p) acc = fma(M[tri(NU + p) + jj], row[NU + p], acc);
                row[jj] = -acc;
            }
            __syncthreads();
            for (int jj = NU - 1; jj >= 0; --jj) {
                if (tid < RT_NPAR) M[tri(NZ + 1 + tid) + jj] /= M[tri(jj) + jj];
                __syncthreads();
                for (int e = tid; e < jj * RT_NPAR; e += RT_BLOCK) {
                    const int i = e / RT_NPAR, j = e % RT_NPAR;
                    double* row = M + tri(NZ + 1 + j);
                    row[i] = fma(-M[tri(jj) + i], row[jj], row[i]);
                }
                __syncthreads();
            }
        }
    }

    // ---- P6: state trajectory X_{k+1} = X_k + dt_k (A X_k + Bj U_jb + Bt v_tb + c), outputs
    double* sX = s.x;
    if (tid < NX) sX[tid] = s.in[VSMPC_IN_X0 + tid];
    __syncthreads();
    for (int k = 0; k < d.n; ++k) {
        if (tid < NX) {
            const int r = tid;
            const double* U = z + NJ * rt_joint_block(d, k);
            const double* V = zv + NTH * rt_throttle_block(d, k);
            double a = sC[r];
            for (int q = 0; q < NJ; ++q) a = fma(sBj[r * NJ + q], U[q], a);
            for (int q = 0; q < NTH; ++q) a = fma(sBt[r * NTH + q], V[q], a);
            for (int q = 0; q < NX; ++q) a = fma(sA[r * NX + q], sX[k * NX + q], a);
            sX[(k + 1) * NX + r] = fma(s.dt[k], a, sX[k * NX + r]);
        }
        __syncthreads();
    }

    // ---- P6 (SENS): dX_{k+1} = dX_k + dt_k (A dX_k + Bj dU_jb + Bt dV_tb), dX_0 = I, into the state rows of dx_dx0 and
    // the node-1 thrust rows of dfm_dx0
    if constexpr (SENS) {
        if (sens_ok) {
            double* DX = s.big;   // dX_k | dX_{k+1}, [26][26] each (K is no longer needed)
            for (int e = tid; e < NX * RT_NPAR; e += RT_BLOCK) DX[e] = e / RT_NPAR == e % RT_NPAR ? 1.0 : 0.0;
            __syncthreads();
            for (int k = 0; k < d.n; ++k) {
                const double* cur = DX + (k & 1) * NX * RT_NPAR;
                double* nxt = DX + ((k + 1) & 1) * NX * RT_NPAR;
                const int ub = NJ * rt_joint_block(d, k), vb = NU + NTH * rt_throttle_block(d, k);
                for (int e = tid; e < NX * RT_NPAR; e += RT_BLOCK) {
                    const int r = e / RT_NPAR, j = e % RT_NPAR;
                    const double* dz = M + tri(NZ + 1 + j);
                    double a = 0.0;
                    for (int q = 0; q < NJ; ++q) a = fma(sBj[r * NJ + q], dz[ub + q], a);
                    for (int q = 0; q < NTH; ++q) a = fma(sBt[r * NTH + q], dz[vb + q], a);
                    for (int q = 0; q < NX; ++q) a = fma(sA[r * NX + q], cur[q * RT_NPAR + j], a);
                    const double v = fma(s.dt[k], a, cur[e]);
                    nxt[e] = v;
                    if (dxout != nullptr) dxout[size_t(inst) * d.nvar * RT_NPAR + size_t(k + 1) * NX * RT_NPAR + e] = v;
                    if (k == 0 && dfmout != nullptr && r >= 12 && r < 20)     // thrust and thrust rate of node 1
                        dfmout[size_t(inst) * VSMPC_FM_SIZE * RT_NPAR + (VSMPC_FM_THRUST + r - 12) * RT_NPAR + j] = v;
                }
                __syncthreads();
            }
        }
    }
    const int iters = s.flags[F_ITERS];
    const int status = bad ? VSMPC_STATUS_NUMERICAL : s.flags[F_STATUS];
    if (xout != nullptr) {
        double* xo = xout + size_t(inst) * d.nvar;
        for (int i = tid; i < d.nxs; i += RT_BLOCK) xo[i] = sX[i];
        for (int i = tid; i < NZ; i += RT_BLOCK) xo[d.nxs + i] = bad ? 0.0 : z[i];
    }
    if (fmout != nullptr && tid < VSMPC_FM_SIZE) {
        double v;
        if (tid < 8) v = z[tid];                                      // delta q           (variableSamplingMPC.cpp:99)
        else if (tid < 12) v = zv[tid - 8];                           // v0                (:100)
        else if (tid < 16) v = Jet::throttle_of_v(zv[tid - 12]);      // throttle %        (:146-149)
        else if (tid < 20) v = sX[NX + 12 + (tid - 16)];              // thrust, node 1    (:101)
        else v = sX[NX + 16 + (tid - 20)];                            // thrust rate, node 1 (:102)
        fmout[size_t(inst) * VSMPC_FM_SIZE + tid] = v;
    }
    if (tid == 0) {
        status_out[inst] = status;
        if (iters_out != nullptr) iters_out[inst] = bad ? 0 : iters;
    }
    if constexpr (SENS) {
        // dx_dx0: dX_0 = I and the joint / throttle rows (P6 wrote the state rows of nodes 1..N); zero unless Solved
        if (dxout != nullptr) {
            double* o = dxout + size_t(inst) * d.nvar * RT_NPAR;
            for (int e = tid; e < NX * RT_NPAR; e += RT_BLOCK) o[e] = sens_ok && e / RT_NPAR == e % RT_NPAR ? 1.0 : 0.0;
            if (!sens_ok)
                for (int e = NX * RT_NPAR + tid; e < d.nxs * RT_NPAR; e += RT_BLOCK) o[e] = 0.0;
            for (int e = tid; e < NZ * RT_NPAR; e += RT_BLOCK) {
                const int c = e / RT_NPAR, j = e % RT_NPAR;
                o[size_t(d.nxs) * RT_NPAR + e] = sens_ok ? M[tri(NZ + 1 + j) + c] : 0.0;
            }
        }
        // dfm_dx0: joint increments, v0 and throttle percent (P6 wrote the node-1 thrust rows)
        if (dfmout != nullptr) {
            double* o = dfmout + size_t(inst) * VSMPC_FM_SIZE * RT_NPAR;
            for (int e = tid; e < VSMPC_FM_THRUST * RT_NPAR; e += RT_BLOCK) {
                const int r = e / RT_NPAR, j = e % RT_NPAR;
                const double* dz = M + tri(NZ + 1 + j);
                double v = 0.0;
                if (sens_ok) {
                    if (r < 8) v = dz[r];
                    else if (r < 12) v = dz[NU + r - 8];
                    else v = Jet::dthrottle_dv(zv[r - 12]) * dz[NU + r - 12];
                }
                o[e] = v;
            }
            if (!sens_ok)
                for (int e = VSMPC_FM_THRUST * RT_NPAR + tid; e < VSMPC_FM_SIZE * RT_NPAR; e += RT_BLOCK) o[e] = 0.0;
        }
        if (active_out != nullptr)
            for (int p = tid; p < NV; p += RT_BLOCK)
                active_out[size_t(inst) * NV + p] = !factored ? 0 : ((hold && p < NTH) ? 2 : s.state[p]);
        if (tid == 0 && flags_out != nullptr) {
            int fl = VSMPC_SENS_UNSOLVED;
            if (sens_ok) {   // weakly or nearly active non-pinned throttles: the Jacobian is one-sided there
                fl = 0;
                double smax = 0.0;
                for (int p = 0; p < NV; ++p) smax = fmax(smax, fabs(sS[p]));
                const double gt = VSMPC_SENS_GRAD_TOL * (1.0 + smax);
                for (int p = 0; p < NV; ++p) {
                    if (hold && p < NTH) continue;
                    const int st = s.state[p];
                    const double v = zv[p], bt = VSMPC_SENS_BOUND_TOL * (1.0 + fabs(v));
                    if ((st != 0 && fabs(s.vec2[p]) <= gt) || (st == 0 && (v - vmin <= bt || vmax - v <= bt)))
                        fl |= VSMPC_SENS_DEGENERATE;
                }
            }
            flags_out[inst] = fl;
        }
    }
