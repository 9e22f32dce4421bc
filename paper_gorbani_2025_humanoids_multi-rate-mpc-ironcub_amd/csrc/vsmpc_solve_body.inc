// Body of the solve kernels, P0 to P6: the text between the braces of solve_kernel, solve_kernel_tuned and
// solve_kernel_small (vsmpc_kernels.hip).
//
// The includer declares, as template parameters, constants or kernel arguments:
//   D       Dims<nIter, nIterSmall, controlHorizon>
//   STAMPS  bool: the diagnostic instantiation (phase stamps, t_acc, the debug dumps)
//   FORM    int: how P1 condenses, 0 = SYRK form, 1 = structured form (PIPE below; needs D::STRUCT_P1)
//   TUNED   bool: P0 takes the weights and limits from the instance's row of `tun` instead of `cfg`
//   SMALL   bool: the small-batch kind (FORM 1 and !TUNED only): Smem<D, true>, tiles formed beside the first panel streams
//   cfg, in, batch, tun   kernel arguments (tun: a null constant where !TUNED)
// and its arguments begin as SolveArgs does: everything behind `batch` is read through late_args().
// Macros: VS_STAMP, VS_TIC, VS_TOC, VS_REFRESH_IDS and VS_P6_TOC are defined here and undefined at the end; VS_DIAG_QP,
// VS_DIAG_P3 and VS_DIAG_P6 (measurement builds, from the command line) are read.
//
// Textual on purpose: the same text inlined from a device function is not the same kernel (three signatures tried: -3
// instructions in solve_kernel<Dims<17,7,12>, false, 0>, -6 in <.., false, 1>; tools/isa_diff.py), and which of the two is
// faster nobody has measured.  Sharing inside the body is by lambdas, each checked the same way.
#define VS_STAMP(i)                                                                        \
    do {                                                                                    \
        if constexpr (STAMPS) {                                                             \
            unsigned long long* st_ = late_args()->stamps;                                  \
            if (tid == 0 && st_ != nullptr) st_[size_t(blockIdx.x) * 16 + (i)] = __builtin_amdgcn_s_memtime(); \
        }                                                                                   \
    } while (0)
    unsigned long long t_acc[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long t_mark = 0, stamp_t1 = 0, rt0 = 0;
    if constexpr (STAMPS) rt0 = __builtin_amdgcn_s_memrealtime();  // constant 100 MHz clock: wall time of this instance
#define VS_TIC()                                                     \
    do {                                                             \
        if constexpr (STAMPS) t_mark = __builtin_amdgcn_s_memtime(); \
    } while (0)
#define VS_TOC(i)                                                          \
    do {                                                                   \
        if constexpr (STAMPS) {                                            \
            const unsigned long long t_now = __builtin_amdgcn_s_memtime(); \
            t_acc[i] += t_now - t_mark;                                    \
            t_mark = t_now;                                                \
        }                                                                  \
    } while (0)
    using S = Smem<D, SMALL>;   // (SMALL moves the arrays of P1a / P1s only)
    static_assert(!SMALL || (FORM == 1 && !TUNED), "the small-batch kind is the structured form of the shared kind");
    // The structured form: its tile entries, P2 and P3 sit behind one wave dispatch (see P1); P3 runs pipelined -- wavefront 0
    // factors the panels, wavefronts 1..3 hold all tiles (TileTab, cholesky_wave) -- so wavefront 0 runs the jets link of P6
    // beside P5, and P6 starts at the momenta
    constexpr bool PIPE = FORM == 1;
    // steps of the joint reduction that run in P0 (wavefront 3); the rest follows a generator chain in P1.  Long horizons
    // have ~9 k cycles of slack behind the generator chains, short ones ~3 k.
    constexpr int QR_P0_STEPS = D::STRUCT_LONG ? 1 : 2;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* sIn = smem + S::oIn;
    double* sA = smem + S::oA;
    double* sBj = smem + S::oBj;
    double* sBt = smem + S::oBt;
    double* sC = smem + S::oC;
    double* sVprev = smem + S::oVprev;
    double* sInvD = smem + S::oInvD;
    double* sW = smem + S::oW;
    double* sZ = smem + S::oZ;
    double* sSv = smem + S::oSv;
    double* sSvec = smem + S::oSvec;
    double* sV = smem + S::oV;
    double* sX = smem + S::oX;
    double* sF = smem + S::oF;
    double* sDt = smem + S::oDt;
    double* sCfg = smem + S::oCfg;
    int* sFlags = reinterpret_cast<int*>(smem + S::oFlags);  // [0] numerical failure, [1] status, [2] iters, [3] bound violated, [4] which
    double* sY = smem + S::oY;
    double* Lb = smem + S::oM;        // tile storage: ring of two panel columns + throttle corner (see Dims)
    double* sXinv = smem + S::oXinv;  // inverses of the joint diagonal tiles and of the first throttle tile
    double* sQP = smem + S::oQP;      // dual box QP work arrays
    double* sU = smem + S::oU;        // register back-substitution: per-wavefront partial sums, scratch

    // Work-item ids are RE-DERIVED at every phase boundary (VS_REFRESH_IDS: lane from v_mbcnt behind an opaque operand,
    // wave from its scalar register) instead of being carried through the kernel: a value that is live from the first
    // to the last instruction is the register allocator's favourite spill candidate, and every reload from scratch is a
    // global-memory round trip on the critical path of a latency-bound workgroup.
    const int inst = blockIdx.x;
    if (inst >= batch) return;
    int tid = threadIdx.x;
    int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: wave-dependent branches become s_cbranch
    // (Rotating which hardware wavefront plays which role with the workgroup index -- so that the serial role-0 phases of two
    // co-resident workgroups do not share a SIMD -- measured no different at batch 4096: 392.3 us against 388.1.)
#define VS_REFRESH_IDS()                                                                     \
    do {                                                                                     \
        unsigned m_ = ~0u;                                                                   \
        asm volatile("" : "+s"(m_));                                                         \
        lane = int(__builtin_amdgcn_mbcnt_hi(m_, __builtin_amdgcn_mbcnt_lo(m_, 0u)));        \
        tid = (wave << 6) | lane;                                                            \
    } while (0)

    // tiles of the lower triangle are dealt round-robin to the wavefronts: tile t -> wave t % NWAVES, slot t / NWAVES
    // (stage-sorted table in constant memory, padded with never-active dummies)
    constexpr int TPW = TileTab<D, PIPE>::TPW;

    VS_STAMP(0);
    // ---------------------------------------------------------------- P0
    {   // 16 B per lane: the record stride (NIN doubles) and the LDS base are multiples of 16 B
        static_assert(D::NIN % 2 == 0 && D::NVAR % 2 == 0 && D::NXS % 2 == 0 && D::NUO % 2 == 0, "double2 I/O");
        // the record's HBM round trip (~1 us) is overlapped with the LDS initialisation: loads first, dependent stores last
        static_assert(D::NIN / 2 <= D::BLOCK, "one 16-byte load per thread covers the record");
        const double2* in2 = reinterpret_cast<const double2*>(in + size_t(inst) * D::NIN);
        double2* sIn2 = reinterpret_cast<double2*>(sIn);
        double2 rec = make_double2(0.0, 0.0);
        if (tid < D::NIN / 2) rec = in2[tid];
        // the instance's row of tunables rides in the same window: 16 lanes x 16 B, the last lanes of the workgroup
        constexpr int TUN0 = D::BLOCK - CFG_SIZE / 2;
        double2 trow = make_double2(0.0, 0.0);
        if constexpr (TUNED) {
            static_assert(CFG_SIZE == VSMPC_TUNE_SIZE && CFG_SIZE % 2 == 0 && CFG_VMAX == CFG_SIZE - 2, "row = sCfg + one pad");
            if (tid >= TUN0) trow = reinterpret_cast<const double2*>(tun + size_t(inst) * CFG_SIZE)[tid - TUN0];
        }
        if (tid < 4) sFlags[tid] = 0;
        if (tid < D::N) sDt[tid] = cfg.dt[tid];
        if constexpr (!TUNED) {
            if (tid >= 64 && tid < 64 + NWROWS) sCfg[CFG_SQ + tid - 64] = cfg.sq[tid - 64];
            if (tid >= 96 && tid < 96 + NJ) sCfg[CFG_WJ + tid - 96] = cfg.wj[tid - 96];
            if (tid == 128) {
                sCfg[CFG_WREG] = cfg.w_reg; sCfg[CFG_WTHR] = cfg.w_thr; sCfg[CFG_WINIT] = cfg.w_init;
                sCfg[CFG_VMIN] = cfg.vmin; sCfg[CFG_VMAX] = cfg.vmax;
            }
        }
        for (int i = tid; i < NX * NX + NX * NJ + NX * NTH + 28; i += D::BLOCK) sA[i] = 0.0;  // A,Bj,Bt,c contiguous
        if (tid < D::NIN / 2) sIn2[tid] = rec;
        if constexpr (TUNED) {
            if (tid >= TUN0) {
                sCfg[2 * (tid - TUN0)] = trow.x;
                sCfg[2 * (tid - TUN0) + 1] = trow.y;
            }
            // a non-finite tunable ends like a non-finite record: status Numerical (the pad entry of the row is not looked at)
            const bool fin = isfinite(trow.x) && (isfinite(trow.y) || tid == D::BLOCK - 1);
            __syncthreads();
            if (!fin) sFlags[0] = 1;
        } else {
            __syncthreads();
        }
    }
    p0_linearize<false, false, false>(cfg.use_jet, sIn, sA, sBj, sBt, sC, sVprev, tid, D::BLOCK);  // barrier: after P1a below
    // joint reduction: 6 unknowns per joint block instead of 8 (NJC).  The SYRK form needs the reduced input matrix at the top
    // of its recursion: all six steps here, in wavefront 3, which has only copies to do in P0 (5.6 k cycles, of which ~2.8 k
    // lengthen P0).  The structured form needs it for the tile entries only: three steps here (hidden), the other three in a
    // generator wavefront after its chain, in the ~3 k cycles it would otherwise wait for the throttle wavefronts (below).
    if (wave == 3) {
        if constexpr (FORM == 1) p0_joint_reduction<D, 0, QR_P0_STEPS>(smem, lane);
        else p0_joint_reduction<D>(smem, lane);
    }

    // P1a: jet sub-system.  The model is a cascade (jets -> momenta -> CoM / RPY -> integrators) and the jets are
    // decoupled from each other, so of the condensed columns only the throttle columns (one jet each) and the affine
    // column (four) carry a non-zero thrust sensitivity: NV + 4 two-state recursions over the whole horizon, one per
    // lane, whose thrust trajectories T_k go to LDS.  The momentum recursion below then needs one scalar per column and
    // stage instead of eight jet states, their input vectors and twelve coefficients in every thread -- which is what
    // brings P1 under the 256 registers a wavefront gets when two workgroups share a CU.   (systemDynamicsVSMPC.cpp:384-429)
    constexpr int NJROW = D::NV + NTH + 1, ZROW = D::NV + NTH;  // + an all-zero row for the joint and padding columns
    double* sJetT = sXinv;                    // [NJROW][N]; the X tiles are not written before P3
    if constexpr (SMALL) sJetT = smem + S::oJetT;   // (the small-batch kind keeps it apart from them)
    static_assert(SMALL || S::oJetT == S::oXinv, "the jet trajectories lie at the head of the X region");
    double* sGA = sJetT + NJROW * D::N;       // [2][N][3]: A_mom T_k of the affine column, per half
    static_assert(D::NV + NTH <= 64 && (SMALL || NJROW * D::N + 6 * D::N <= S::NXT * D::TS), "jet trajectories fit the X region");
    // Runs in the wavefront whose lanes 0..3 linearised the jets (p0_linearize), straight behind that, while the other
    // wavefronts finish their pieces of P0: LDS operations of one wavefront execute in order, no barrier needed.
    if (wave == 1) {
        if (lane < D::NV + NTH) {
            const bool affl = lane >= D::NV;
            const int i = affl ? lane - D::NV : (lane & 3);
            const int blk = affl ? -1 : v_block_of_internal<D>(lane);
            const double jon = sA[(12 + i) * NX + 16 + i], ja = sA[(16 + i) * NX + 12 + i], jb = sA[(16 + i) * NX + 16 + i];
            const double c12 = sC[12 + i], c16 = sC[16 + i], b12 = sBt[(12 + i) * NTH + i], b16 = sBt[(16 + i) * NTH + i];
            const double t0 = sIn[VSMPC_IN_X0 + 12 + i], td0 = sIn[VSMPC_IN_X0 + 16 + i];
            const double bT = affl ? c12 : b12, bTd = affl ? c16 : b16;
            double T = affl ? t0 : 0.0, Td = affl ? td0 : 0.0;
#pragma unroll
            for (int k = 0; k < D::N; ++k) {
                sJetT[lane * D::N + k] = T;   // the momentum rate of stage k sees T_k (explicit Euler)
                const double mT = (affl || throttle_block_of_stage<D>(k) == blk) ? 1.0 : 0.0;
                const double dT = fma(jon, Td, mT * bT);
                const double dTd = fma(ja, T, fma(jb, Td, mT * bTd));
                const double dt = sDt[k];
                T = fma(dt, dT, T);
                Td = fma(dt, dTd, Td);
            }
        }
        for (int k = lane; k < D::N; k += 64) sJetT[ZROW * D::N + k] = 0.0;
        if constexpr (FORM == 1) {
            // P1s: the affine column's whole momentum forcing A_mom Tbar_k + c_h, straight behind the trajectories it reads (same
            // wavefront: LDS operations stay in order) and from the record instead of the linearisation the other wavefronts
            // are still writing -- A_mom as p0_linearize copies it, c_h = alpha m R^T g as it forms it -- so that P0 needs no
            // second block behind a second barrier (v30; was: all threads, after the barrier below, then another one)
            const double am = sIn[VSMPC_IN_ALPHA] * sIn[VSMPC_IN_MASS];
            const double* R = sIn + VSMPC_IN_WRB;
            const double* gr = sIn + VSMPC_IN_GRAV;
            for (int e = lane; e < 6 * D::N; e += 64) {
                const int h = e / (3 * D::N), k = (e / 3) % D::N, r = e % 3;
                double g = 0.0;
#pragma unroll
                for (int c = 0; c < NTH; ++c) g = fma(sIn[VSMPC_IN_AMOM + (3 * h + r) * NTH + c], sJetT[(D::NV + c) * D::N + k], g);
                const double ch = h == 0 ? am * (R[0 + r] * gr[0] + R[3 + r] * gr[1] + R[6 + r] * gr[2]) : 0.0;
                sGA[e] = g + ch;
            }
        }
    }
    if constexpr (FORM == 1) {
        // the zeros and the reference window (+ c_e = -p_ref / -rpy_init on the CoM / RPY rows, as p0_linearize writes it) by the
        // wavefront whose lane 0 does the scalar CoM / gravity piece of the linearisation: none of it waits for anything
        if (wave == 2) {
            for (int e = lane; e < S::sizeZero; e += 64) smem[S::oSZero + e] = 0.0;
            for (int e = lane; e < 12 * D::NREF; e += 64) {
                const int row = e % 12;
                const double off = row < 3 ? -sIn[VSMPC_IN_PREF + row] : ((row >= 6 && row < 9) ? -sIn[VSMPC_IN_RPYINIT + row - 6] : 0.0);
                smem[S::oSRefC + e] = sIn[VSMPC_IN_XREF + e] + off;
            }
        }
    }
    if constexpr (FORM == 1 && D::STRUCT_LONG) {   // the chains ADD into sAc (30 KB at the 2x horizon: all threads)
        for (int e = tid; e < S::sizeAc; e += D::BLOCK) smem[S::oSAc + e] = 0.0;
    }
    __syncthreads();   // ends P0 and the jet trajectories
    if constexpr (FORM != 1) {
        for (int e = tid; e < 6 * D::N; e += D::BLOCK) {
            const int h = e / (3 * D::N), k = (e / 3) % D::N, r = e % 3, row = (h ? 9 : 3) + r;
            double g = 0.0;
#pragma unroll
            for (int c = 0; c < NTH; ++c) g = fma(sA[row * NX + 12 + c], sJetT[(D::NV + c) * D::N + k], g);
            sGA[e] = g;
        }
        __syncthreads();
    }

    VS_STAMP(1);
    VS_REFRESH_IDS();
    if constexpr (STAMPS) stamp_t1 = __builtin_amdgcn_s_memtime();
    // ---------------------------------------------------------------- P1 condense
    d4 acc[TPW];
    if constexpr (FORM == 1) {
        // P1s: structured condensing.  Generator lanes on wavefronts 0 / 1 (linear / angular half), throttle and affine
        // columns on wavefronts 2 / 3; no communication inside the chains, one barrier, then the entries of the owned
        // tiles straight into the accumulator registers.
        static_assert(D::STRUCT_P1, "structured condensing is instantiated for horizons with Dims::STRUCT_P1");
        VS_TIC();
        if (wave < 2) {
            p1s_chain<D, 0, SMALL>(cfg, wave, lane, smem);
            if (wave == 0) p0_joint_reduction<D, QR_P0_STEPS, NJC>(smem, lane);   // (second half; writes Bj and sQR, which nobody touches
                                                                        // before the barrier below)
        } else {
            p1s_chain<D, 1, SMALL>(cfg, wave - 2, lane, smem);
        }
        VS_TOC(0);
        __syncthreads();
        VS_TOC(1);
        // (the small-batch kind forms sAc beside panel stream 0, in wavefronts 1..3: nothing in front of that stream reads it,
        // and this barrier is not on its path -- small_form, instalment 1)
        if constexpr (!D::STRUCT_LONG && !SMALL) {
            p1s_contract<D>(smem, tid);
            __syncthreads();
        }
        VS_TOC(3);
        // ONE wave dispatch for the entries, P2 and P3 -- the accumulator tiles are born and factored inside one branch, no join
        // in between (at a join the allocator moved the tiles of a wavefront through the vector registers, and at the 2x
        // horizon pushed other values into scratch to make room).  The diagnostic instantiation takes the same path; its
        // dumps -- condensed Hessian before, factor after P3 -- and the stamps of the P1 / P2 / P3 boundaries sit inside the
        // branch.
        auto tail = [&](auto wcst) __attribute__((always_inline)) {
            constexpr int W = decltype(wcst)::value;
            if constexpr (SMALL) {
                // only tile column 0, dealt over the four wavefronts, P2 term and hand-over to LDS included; the other
                // tiles are formed beside the first two panel streams (cholesky_wave).  Stamps 2 and 3 therefore both
                // mark "column 0 is in the ring": the rest of the entries and of P2 lies between stamps 3 and 4.
                static_for<0, TPW>([&](auto qcst) __attribute__((always_inline)) {
                    constexpr int q = decltype(qcst)::value;
                    if constexpr (small_instalment<D, TPW, W>(q) < 0) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
                });
                const int ln0 = fresh_lane();
                small_form<D, TPW, W, 0>(sCfg, acc, Lb, smem + S::oQR + S::QR_GY, sVprev, ln0, (ln0 >> 4) * 17 + (ln0 & 15));
            } else {
                p1s_entries<D, TPW, W, PIPE>(acc, smem, lane);
            }
            VS_TOC(2);
            __syncthreads();   // the LDS arrays of P1s lie under the ring P3 is about to fill (not in the small-batch kind, where
                               // this is the barrier behind instalment 0 and the only one in front of stream 0)
            VS_STAMP(2);
            constexpr TileTab<D, PIPE> tab{};
            double* dbgLw = nullptr;
            if constexpr (STAMPS && !SMALL) {   // (a dump needs all tiles at one point: the launcher asks the shipped kernel)
                double* dbgM = late_args()->dbgM;
                double* dbgL = late_args()->dbgL;
                dbgLw = dbgL != nullptr ? dbgL + size_t(inst) * D::NP * D::NP : nullptr;
                if (dbgM != nullptr) {
                    const int ln = fresh_lane();
                    static_for<0, TPW>([&](auto qcst) __attribute__((always_inline)) {
                        constexpr int q = decltype(qcst)::value;
                        constexpr int t = q * D::NWAVES + W;
                        if constexpr (tab.forms(t, W))
                            dump_hessian_tile<D>(dbgM + size_t(inst) * D::NP * D::NP, tab.ti[t], tab.tj[t], acc[q], sCfg,
                                                 smem + S::oQR + S::QR_GY, sVprev, ln);
                    });
                }
            }
            VS_STAMP(3);
            if constexpr (D::WG_PER_CU == 1) pin_tiles_agpr<TPW>(acc);
            const int ln = fresh_lane();
            cholesky_wave<D, TPW, W, STAMPS, PIPE, SMALL>(sCfg, acc, Lb, sInvD, smem + S::oQR + S::QR_GY, sVprev, sFlags, sXinv, sW, dbgLw, ln,
                                                  (ln >> 4) * 17 + (ln & 15), (ln & 15) * 17 + (ln >> 4), sZ);
            if constexpr (STAMPS) {
                if (dbgLw != nullptr) {
                    const int l2 = fresh_lane();
                    static_for<0, TPW>([&](auto qcst) __attribute__((always_inline)) {
                        constexpr int q = decltype(qcst)::value;
                        constexpr int t = q * D::NWAVES + W;
                        if constexpr (tab.holds(t, W) && tab.tj[t] < D::PVT && tab.ti[t] > tab.tj[t])
                            dump_factor_tile<D>(dbgLw, tab.ti[t], tab.tj[t], acc[q], l2);
                    });
                }
            }
        };
        switch (wave) {
            case 0: tail(std::integral_constant<int, 0>{}); break;
            case 1: tail(std::integral_constant<int, 1>{}); break;
            case 2: tail(std::integral_constant<int, 2>{}); break;
            default: tail(std::integral_constant<int, 3>{}); break;
        }
    } else {
#pragma unroll
        for (int q = 0; q < TPW; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
        // P1b: thread (half, c): half 0 = linear part (p, h_lin, e_pos), half 1 = angular part (rpy, h_ang, e_rpy) of the
        // condensed columns c, c + 128, ... (CPT of them; one at the paper horizon).  Same code, different coefficient rows.
        constexpr int CPT = D::CPT;
        // every wavefront runs the recursion of a pass, then its share of the SYRK
        const int pw = wave;
        const int ptid = tid;
        const int half = pw / (D::NWAVES / 2);  // scalar
        const int xr0 = half ? 6 : 0, hr0 = half ? 9 : 3, er0 = half ? 23 : 20;  // state rows
        const int yx0 = half ? 6 : 0, yh0 = half ? 9 : 3, ye0 = half ? 15 : 12;  // weighted-row slots

        // coefficient rows of this half: wave-uniform LDS broadcasts, re-read at the top of every pass so that they are
        // dead during the matrix-core section (the accumulator tiles stay in registers for the whole of P1..P5)
        double M1[9], Sk[9], Ce[3], sqx[3], sqh[3], sqe[3];
        auto load_coeffs = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    M1[3 * r + c] = sA[(xr0 + r) * NX + hr0 + c];
                    Sk[3 * r + c] = sA[(hr0 + r) * NX + hr0 + c];
                }
                Ce[r] = sC[er0 + r];
                sqx[r] = sCfg[CFG_SQ + yx0 + r];
                sqh[r] = sCfg[CFG_SQ + yh0 + r];
                sqe[r] = sCfg[CFG_SQ + ye0 + r];
            }
        };
        // MFMA operand addresses: lane l reads Y[4 ks + (l >> 4)][16 tile + (l & 15)]; the k-step enters as an
        // immediate offset of ds_read_b64
        const int ylane = (lane >> 4) * D::YS + (lane & 15);
        constexpr int NPASS = (D::N + 1) / 2;
        if constexpr (STAMPS) { t_mark = stamp_t1; VS_TOC(3); }  // P1 set-up

        // The sensitivity recursion over the whole horizon + the SYRK into all accumulator slots of this wavefront.
        // Y is single-buffered (two barriers per pass): the second buffer is what kept a second workgroup off the CU,
        // and a co-resident workgroup fills the recursion's bubbles far better than the look-ahead did.
        int col[CPT], kind[CPT], blk[CPT];   // kind: 0 joint column, 1 throttle column, 2 affine column, 3 pad
        double aff[CPT], xs[CPT][3], hs[CPT][3], es[CPT][3], bha[CPT][3];
        const double* jetT[CPT];
        const double* gaT = sGA + half * 3 * D::N;
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) {
            const int c = cc * D::PCOLS + ptid % D::PCOLS;
            int comp = 0;
            col[cc] = c;
            kind[cc] = 3;
            blk[cc] = 0;
            if (c < D::NUY) { kind[cc] = 0; blk[cc] = c / NJC; comp = c - NJC * blk[cc]; }   // (dummy unknowns: kind 3)
            else if (c >= D::NU && c < D::NZ) { kind[cc] = 1; blk[cc] = v_block_of_internal<D>(c - D::NU); comp = (c - D::NU) & 3; }
            else if (c == D::NZ) { kind[cc] = 2; }
            // unconditional loads (every address is valid for every column), selected afterwards: conditional loads
            // become branches and the LDS latencies add up instead of overlapping
            const int jc = comp & 7, tc = comp & 3;
            const bool aff_col = kind[cc] == 2, jnt_col = kind[cc] == 0, thr_col = kind[cc] == 1;
            aff[cc] = aff_col ? 1.0 : 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double x0 = sIn[VSMPC_IN_X0 + xr0 + r], h0 = sIn[VSMPC_IN_X0 + hr0 + r], e0 = sIn[VSMPC_IN_X0 + er0 + r];
                const double bj = sBj[(hr0 + r) * NJ + jc], ch = sC[hr0 + r], at = sA[(hr0 + r) * NX + 12 + tc];
                xs[cc][r] = aff_col ? x0 : 0.0;
                hs[cc][r] = aff_col ? h0 : 0.0;
                es[cc][r] = aff_col ? e0 : 0.0;
                // one input vector per column: joint column -> Bj column (scaled by the block activity), affine column -> c
                // (always on), throttle column -> thrust map column of the one jet it drives (scaled by that jet's T_k)
                bha[cc][r] = jnt_col ? bj : (aff_col ? ch : (thr_col ? at : 0.0));
            }
            // this column's thrust trajectory: a throttle column's own jet, the zero row otherwise (the affine column's
            // four jets enter through sGA)
            jetT[cc] = sJetT + (thr_col ? c - D::NU : ZROW) * D::N;
        }
        // wave-uniform tile coordinates of the slots, packed two slots per scalar register (see TilePack)
        unsigned tpk[TilePack<D>::NWORDS];
#pragma unroll
        for (int k = 0; k < TilePack<D>::NWORDS; ++k) tpk[k] = kTilePack<D>.w[pw][k];
        const double* ybase = sY + ylane;   // + the buffer of the pass (latency form: two Y buffers)
        constexpr bool UNROLLED = TPW <= SYRK_UNROLL_TPW;
        // In a rolled pass loop the operand addresses are loop invariants: the compiler hoists all 2 TPW of them out of the
        // loop and, at 30 slots, spills them -- ~4k cycles of scratch reloads per pass (measured).  The packed word is
        // therefore made opaque where it is used: one shift-and-add per operand address, in place.
        auto slot_word = [&](int q) __attribute__((always_inline)) {
            unsigned w = tpk[q >> 1];
            if constexpr (!UNROLLED) asm volatile("" : "+s"(w));
            return w;
        };
        auto slot_a = [&](int q) __attribute__((always_inline)) { return ybase + 16 * int((slot_word(q) >> (16 * (q & 1))) & 0xffu); };
        auto slot_b = [&](int q) __attribute__((always_inline)) { return ybase + 16 * int((slot_word(q) >> (16 * (q & 1) + 8)) & 0xffu); };
        // one pass of the recursion (nodes 2m, 2m + 1 -> the Y buffer sYm) and one pass of the SYRK (Y buffer behind ybase)
        auto rec_pass = [&](int m, int nnodes, double* sYm) __attribute__((always_inline)) {
            load_coeffs();
#pragma unroll
            for (int par = 0; par < 2; ++par) {
                if (par >= nnodes) break;  // the last pass of an odd horizon has one node
                const int k = 2 * m + par;  // stage k -> node k+1
                const double dt = sDt[k];
                // reference of this node (affine column only; column map costsVSMPC.cpp:191-200) and the affine column's
                // thrust forcing, requested before the recursion so that the LDS latency is spent under it
                const int rc = k < D::NS ? 0 : k - D::NS;
                const double* xr = sIn + VSMPC_IN_XREF + rc * 12;  // uniform address: LDS broadcast
                double xrx[3], xrh[3], ga[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) { xrx[r] = xr[yx0 + r]; xrh[r] = xr[yh0 + r]; ga[r] = gaT[3 * k + r]; }
#pragma unroll
                for (int cc = 0; cc < CPT; ++cc) {
                    const double tk = jetT[cc][k];
                    const bool actJ = (kind[cc] == 0 && joint_block_of_stage<D>(k) == blk[cc]) || kind[cc] == 2;
                    // input activity as a 0/1 factor inside the multiply-adds (a 64-bit select costs two instructions)
                    const double scale = kind[cc] == 1 ? tk : (actJ ? 1.0 : 0.0);
                    double dx[3], dh[3], de[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        double a0 = M1[3 * r] * hs[cc][0], a1 = scale * bha[cc][r], a2 = aff[cc] * ga[r];
#pragma unroll
                        for (int c = 1; c < 3; ++c) a0 = fma(M1[3 * r + c], hs[cc][c], a0);
#pragma unroll
                        for (int c = 0; c < 3; ++c) a1 = fma(Sk[3 * r + c], hs[cc][c], a1);
                        dx[r] = a0;
                        dh[r] = a1 + a2;
                        de[r] = fma(aff[cc], Ce[r], xs[cc][r]);
                    }
#pragma unroll
                    for (int r = 0; r < 3; ++r) { xs[cc][r] += dt * dx[r]; hs[cc][r] += dt * dh[r]; es[cc][r] += dt * de[r]; }
                    // Y rows of this node: sqrt(Q) (S_k - xref_k on the affine column); column map costsVSMPC.cpp:191-200
                    if (CPT == 1 || col[cc] < D::NP) {
                        double* Yn = sYm + 18 * par * D::YS + col[cc];
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const double vx = fma(-aff[cc], xrx[r], xs[cc][r]);  // aff = 1 on the affine column, else 0
                            const double vh = fma(-aff[cc], xrh[r], hs[cc][r]);
                            Yn[(yx0 + r) * D::YS] = sqx[r] * vx;
                            Yn[(yh0 + r) * D::YS] = sqh[r] * vh;
                            Yn[(ye0 + r) * D::YS] = sqe[r] * es[cc][r];
                        }
                    }
                }
            }
            if (nnodes == 1)  // rows 18,19 of the last, single-node pass (k-step 4 reads rows 16..19)
                for (int i = ptid; i < 2 * D::YS; i += D::BLOCK) sYm[18 * D::YS + i] = 0.0;
        };
        // Short horizons: the pass loop is UNROLLED and the number of slots a pass runs is a compile-time constant, the same
        // for the four wavefronts (the maximum over them: a wavefront with fewer active tiles multiplies columns of Y
        // that are still exactly zero).  The SYRK of a pass is then straight-line code -- a branch per slot, or any
        // other control flow around the chains, makes the register allocator move whole accumulator tiles at the joins
        // (measured: ~1.1k cycles per pass).  The wavefront with the most active tiles sets the pace either way.
        auto syrk_fixed = [&](auto nks_c, auto nact_c) __attribute__((always_inline)) {
            constexpr int NKS = decltype(nks_c)::value, NACT = decltype(nact_c)::value;
            if constexpr (NACT > 0) {
                double ha[SYRK_DIST], hb[SYRK_DIST];
#pragma unroll
                for (int ks = 0; ks < SYRK_DIST; ++ks) {
                    ha[ks] = slot_a(NACT - 1)[ks * 4 * D::YS];
                    hb[ks] = slot_b(NACT - 1)[ks * 4 * D::YS];
                }
#pragma unroll
                for (int q = NACT - 1; q >= 0; --q) {
                    const int qn = q > 0 ? q - 1 : 0;
                    syrk_slot<D, NKS, true>(acc[q], slot_a(q), slot_b(q), ha, hb, slot_a(qn), slot_b(qn));
                }
            }
        };
        if constexpr (UNROLLED) {
            static_for<0, NPASS>([&](auto mc) __attribute__((always_inline)) {
                constexpr int m = decltype(mc)::value;
                constexpr int nnodes = (2 * m + 1 < D::N) ? 2 : 1;
                VS_TIC();
                rec_pass(m, nnodes, sY);
                VS_TOC(0);
                __syncthreads();
                VS_TOC(1);
                syrk_fixed(std::integral_constant<int, nnodes == 2 ? 9 : 5>{}, std::integral_constant<int, nact_max<D>(m)>{});
                VS_TOC(2);
                __syncthreads();  // single Y buffer: the next pass overwrites it
            });
        } else {
            // long horizons: consecutive passes with the same slot count share one rolled loop whose body is straight-line
            // (see PassGroups): the code stays small (one set of chains per DISTINCT slot count, not per pass)
            static_for<0, PassGroups<D>::count()>([&](auto gc) __attribute__((always_inline)) {
                constexpr PassGroups<D> pg{};
                constexpr int g = decltype(gc)::value;
#pragma unroll 1
                for (int m = pg.start[g]; m < pg.end[g]; ++m) {
                    VS_TIC();
                    rec_pass(m, pg.nks[g] == 9 ? 2 : 1, sY);
                    VS_TOC(0);
                    __syncthreads();
                    VS_TOC(1);
                    syrk_fixed(std::integral_constant<int, pg.nks[g]>{}, std::integral_constant<int, pg.nact[g]>{});
                    VS_TOC(2);
                    __syncthreads();  // single Y buffer: the next pass overwrites it
                }
            });
        }
        VS_TIC();
    }
    VS_REFRESH_IDS();
    if constexpr (D::WG_PER_CU == 1) pin_tiles_agpr<TPW>(acc);   // long horizons: see pin_tiles_agpr

    // ---------------------------------------------------------------- P2 + P3 (wave-specialised, see cholesky_wave)
    static_assert(D::NWAVES == 4, "wave-specialised phases are instantiated for four wavefronts");
    constexpr int PVT = D::PVT;  // first tile row that contains a throttle row
    const int crow = (lane >> 4) * 17 + (lane & 15);  // C/D fragment: row (lane>>4)+4r, column lane&15
    const int lrow = (lane & 15) * 17 + (lane >> 4);  // A/B fragment: row lane&15, k = lane>>4
    // The debug dumps (condensed Hessian, factor; dump_hessian_tile, dump_factor_tile) exist in the diagnostic instantiation
    // only (STAMPS; the launcher picks it when a dump or the stamps are asked for): in the shipped kernel their code --
    // input_cost_term per element, a branch around every store -- cost registers at the joins for nothing.
    double* dbgL = STAMPS ? late_args()->dbgL : nullptr;
    double* dbgLi = dbgL != nullptr ? dbgL + size_t(inst) * D::NP * D::NP : nullptr;
    VS_REFRESH_IDS();   // (crow / lrow keep the derivation above, `lane` below is this one: as shipped)
    if constexpr (!PIPE) {   // the SYRK form's P2 + P3 (the structured form ran them inside its wave dispatch, stamps and dumps included)
        // The dumps look the coordinates up through a copy of `wave` the compiler cannot see through.  With the plain index
        // it based the dword loads of ti / tj of slot 0 on the byte address of valid[wave] (table + wave, offset 3 wave), and
        // a scalar load ignores the low two bits of its base: wavefronts 1..3 dumped slot 0 at another tile's coordinates.
        // (The table is named inside the diagnostic branches only: the shipped units carry no copy of it.)
        int wave_c = wave;
        if constexpr (STAMPS) asm volatile("" : "+s"(wave_c));
        VS_STAMP(2);
        if constexpr (STAMPS) {
            const TileTab<D, PIPE>& tab = kTileTab<D, PIPE>;
            double* dbgM = late_args()->dbgM;
            if (dbgM != nullptr) {
#pragma unroll
                for (int q = 0; q < TPW; ++q) {
                    const int t = q * D::NWAVES + wave, tc = q * D::NWAVES + wave_c;
                    if (tab.forms(t, wave))
                        dump_hessian_tile<D>(dbgM + size_t(inst) * D::NP * D::NP, tab.ti[tc], tab.tj[tc], acc[q], sCfg,
                                             smem + S::oQR + S::QR_GY, sVprev, lane);
                }
            }
        }
        VS_STAMP(3);
        switch (wave) {  // scalar dispatch: every wavefront runs its own straight-line copy, same barrier count
            case 0: cholesky_wave<D, TPW, 0, STAMPS, PIPE>(sCfg, acc, Lb, sInvD, smem + S::oQR + S::QR_GY, sVprev, sFlags, sXinv, sW, dbgLi, lane, crow, lrow, sZ); break;
            case 1: cholesky_wave<D, TPW, 1, STAMPS, PIPE>(sCfg, acc, Lb, sInvD, smem + S::oQR + S::QR_GY, sVprev, sFlags, sXinv, sW, dbgLi, lane, crow, lrow, sZ); break;
            case 2: cholesky_wave<D, TPW, 2, STAMPS, PIPE>(sCfg, acc, Lb, sInvD, smem + S::oQR + S::QR_GY, sVprev, sFlags, sXinv, sW, dbgLi, lane, crow, lrow, sZ); break;
            default: cholesky_wave<D, TPW, 3, STAMPS, PIPE>(sCfg, acc, Lb, sInvD, smem + S::oQR + S::QR_GY, sVprev, sFlags, sXinv, sW, dbgLi, lane, crow, lrow, sZ); break;
        }
        if constexpr (STAMPS) {
            const TileTab<D, PIPE>& tab = kTileTab<D, PIPE>;
            if (dbgLi != nullptr) {
#pragma unroll
                for (int q = 0; q < TPW; ++q) {
                    const int t = q * D::NWAVES + wave, tc = q * D::NWAVES + wave_c;
                    if (tab.holds(t, wave) && tab.tj[tc] < PVT && tab.ti[tc] > tab.tj[tc])
                        dump_factor_tile<D>(dbgLi, tab.ti[tc], tab.tj[tc], acc[q], lane);
                }
            }
        }
    }
    if (STAMPS && dbgLi != nullptr) {
        for (int e = tid; e < (D::NP - 16 * PVT) * (D::NP - 16 * PVT); e += D::BLOCK) {  // throttle corner, from LDS
            const int gr = 16 * PVT + e / (D::NP - 16 * PVT), gc = 16 * PVT + e % (D::NP - 16 * PVT);
            if (gc <= gr) dbgLi[size_t(gr) * D::NP + gc] = Lb[lower_at<D>(gr, gc)];
        }
    }

    VS_STAMP(4);
    VS_REFRESH_IDS();
    if constexpr (D::WG_PER_CU == 1) pin_tiles_agpr<TPW>(acc);
    // ---------------------------------------------------------------- P4/P5 back-substitution L^T z = y
    // Row NZ of the factor holds L^-1 g, so y = -row.  The throttles sit at the end of the order, hence the
    // first tiles of the backward sweep yield the throttles of the QP with only the hold pin enforced.  If
    // they respect their box the sweep simply continues into the joints (active-set iteration 1 of the
    // oracle's rule); otherwise the box QP on the Schur complement runs and the sweep restarts with the
    // throttles prescribed.
    // The joint columns of the factor are in registers by now (their right-hand side entries were put into sW when
    // the tiles came back from the panel); the throttle corner is in LDS, and so is everything the box QP touches.
    const bool hold = sIn[VSMPC_IN_HOLD] != 0.0;
    constexpr int PV = D::PVT;  // first tile that contains a throttle row
    auto init_corner_rhs = [&]() {
        if (tid >= 16 * PV && tid < D::NP) sW[tid] = tid < D::NZ ? -Lb[lower_at<D>(D::NZ, tid)] : 0.0;
    };
    init_corner_rhs();
    if (tid < D::NP) sZ[tid] = (hold && tid >= D::NZ - 4 && tid < D::NZ) ? sVprev[tid - (D::NZ - 4)] : 0.0;
    __syncthreads();

    // behind tile row p of the sweep: its z leaves the right-hand sides of the corner columns to its left (corner columns
    // only: the joint columns are updated from registers in P5)
    auto corner_update = [&](int p) __attribute__((always_inline)) {
        if (p > PV) {
            if (tid >= 16 * PV && tid < 16 * p) {
                const double* T = Lb + tile_off<D>(p, tid >> 4) + (tid & 15);
                const double* zp = sZ + 16 * p;
                double a2 = 0.0;
#pragma unroll
                for (int k = 0; k < 16; ++k) a2 += T[k * 17] * zp[k];
                sW[tid] -= a2;
            }
            __syncthreads();
        }
    };
    // one tile step of the sweep over the corner; `prescribed` = throttles already fixed in sZ
    auto sweep_tile = [&](int p, bool prescribed) {
        if (wave == 0) {
            const int j = lane & 15;  // lane j owns column j of L_pp
            const int gj = 16 * p + j;
            const double* Tpp = Lb + tile_off<D>(p, p) + j;
            double colv[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {  // column j of L_pp; above the diagonal the tile holds leftovers
                const double t = Tpp[k * 17];
                colv[k] = k >= j ? t : 0.0;
            }
            double w = sW[gj];
            // z_j = w_j * inv_eff + zadd: solved rows use 1/L_jj, prescribed rows (pinned or already fixed
            // throttles, gradient row, padding) use inv_eff = 0 and their value; branch-free in the chain
            const bool fix = (gj >= D::NZ) || (gj >= D::NU && (prescribed || (hold && gj >= D::NZ - 4)));
            const double inv_eff = fix ? 0.0 : sInvD[gj];
            const double zadd = (fix && gj < D::NZ) ? sZ[gj] : 0.0;
            double z = 0.0;
#pragma unroll
            for (int k = 15; k >= 0; --k) {
                const double zk = readlane_f64(fma(w, inv_eff, zadd), k);
                z = (j == k) ? zk : z;
                w = fma(-colv[k], zk, w);  // lanes j >= k: colv is zero or w is no longer used
            }
            if (lane < 16) sZ[gj] = z;
        }
        __syncthreads();
        corner_update(p);
    };

    constexpr bool DUALQP = S::DUALQP;
    if constexpr (DUALQP) {
        // The throttle block spans two tile rows.  Last tile row: only its KL = NZ - 16 (NT-1) throttle rows take part
        // (gradient row and padding have z = 0), the hold pins sit here.  First throttle tile row: no pins, and the
        // inverse of its diagonal tile is at hand (X66 from P3), so z = X66^T w needs no chain.
        constexpr int PL = D::NT - 1, KL = D::NZ - 16 * PL;
        static_assert(KL == D::NV - 16 && KL >= 4, "pins live in the last tile row");
        const double* X6 = sXinv + PV * D::TS;
        const double* L76 = Lb + tile_off<D>(PL, PV);
        const double* L77 = Lb + tile_off<D>(PL, PL);
        if (wave == 0) {
            // wavefront 0 runs both throttle tile rows back to back in registers (cross-lane traffic through
            // v_readlane only)
            const int j = lane & 15;
            const int gj = 16 * PL + j;
            const double* Tpp = L77 + j;
            double colv[KL], l76[KL], x6[16];
#pragma unroll
            for (int k = 0; k < KL; ++k) {  // column j of L_pp; above the diagonal the tile holds leftovers
                const double t = Tpp[k * 17];
                colv[k] = k >= j ? t : 0.0;
                l76[k] = L76[k * 17 + j];   // L[16 PL + k][16 PV + j]
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) x6[i] = X6[i * 17 + j];
            double w = sW[gj];
            double w6 = sW[16 * PV + j];
            const bool fix = (j >= KL) || (hold && j >= KL - 4);
            const double inv_eff = fix ? 0.0 : sInvD[gj];
            const double zadd = (fix && j < KL) ? sZ[gj] : 0.0;
            double z = 0.0;
#pragma unroll
            for (int k = KL - 1; k >= 0; --k) {
                const double zk = readlane_f64(fma(w, inv_eff, zadd), k);
                z = (j == k) ? zk : z;
                w = fma(-colv[k], zk, w);
                w6 = fma(-l76[k], zk, w6);  // right-hand side of the first throttle tile row, lane = row
            }
            double z6 = 0.0;                // z = X66^T w6: lane j sums X66[i][j] w6[i]
#pragma unroll
            for (int i = 0; i < 16; ++i) z6 = fma(x6[i], readlane_f64(w6, i), z6);
            if (lane < 16) { sZ[gj] = z; sZ[16 * PV + j] = z6; }
        } else {
            // wavefronts 1..3 meanwhile: the pieces of the dual box QP's set-up (T, X77, s and max |s|), for every instance -- its
            // inputs are final since P3 and its arrays (sQP, sSvec) are not used by anything else before P5.  No barrier
            // inside: the one behind the violation check publishes it.
            dual_setup_beside_sweep<D>(wave, lane);
        }
        // (no barrier here: the only reader of these throttles before the next barrier is the violation check below, in this
        // same wavefront -- LDS operations of one wavefront execute in order)
    } else if constexpr (S::DUAL3) {
        // three throttle tile rows.  Wavefront 1 forms the inverse of the last corner diagonal tile for the box QP beside
        // wavefront 0's sweep (see cholesky_wave for the second one), a few rows in front of every step so that no barrier
        // of the sweep waits for it
        static_assert(D::NT - 1 == PV + 2, "three throttle tile rows");
        double x2[16];
        const double* L22d = Lb + tile_off_c<D>(PV + 2, PV + 2);
        const double* inv2 = sInvD + D::NU + 32;
        if (wave == 1) tile_inverse_rows<0, 8>(L22d, inv2, x2, lane);
        sweep_tile(PV + 2, false);
        // the other two tile rows have no pinned or prescribed entry in this pass and their inverses are at hand (X_PVT from
        // P3, the second one from P3's last panel): z = X^T w, sixteen multiply-adds per lane instead of a 16-step
        // broadcast chain
        auto sweep_tile_x = [&](int p, const double* Xp) {
            if (wave == 0) {
                const int j = lane & 15;
                double z0 = 0.0, z1 = 0.0;
#pragma unroll
                for (int k = 0; k < 16; k += 2) {   // X[k][j] = 0 for k < j (stored zeros); w: uniform addresses
                    z0 = fma(Xp[k * 17 + j], sW[16 * p + k], z0);
                    z1 = fma(Xp[(k + 1) * 17 + j], sW[16 * p + k + 1], z1);
                }
                if (lane < 16) sZ[16 * p + j] = z0 + z1;
            }
            __syncthreads();
            corner_update(p);
        };
        if (wave == 1) tile_inverse_rows<8, 13>(L22d, inv2, x2, lane);
        sweep_tile_x(PV + 1, smem + S::oDual3T0);
        if (wave == 1) {
            tile_inverse_rows<13, 16>(L22d, inv2, x2, lane);
            if (lane < 16) {
#pragma unroll
                for (int i = 0; i < 16; ++i) smem[S::oDual3T1 + i * 17 + lane] = x2[i];
            }
        }
        sweep_tile_x(PV, sXinv + PV * D::TS);
    } else {
#pragma unroll 1
        for (int p = D::NT - 1; p >= PV; --p) sweep_tile(p, false);
    }
    if (wave == 0) {
        const bool valid = lane < D::NV;
        const double v = sZ[D::NU + (valid ? lane : 0)];
        const bool fixed = hold && lane >= D::NV - 4;
        const double tolv = 1e-12 * (1.0 + fabs(v));
        const bool viol = valid && !fixed && (v < sCfg[CFG_VMIN] - tolv || v > sCfg[CFG_VMAX] + tolv);
        const unsigned long long vm = __ballot(viol);
        if (lane == 0) { sFlags[3] = __popcll(vm); sFlags[1] = VSMPC_STATUS_SOLVED; sFlags[2] = 1; }
        if constexpr (DUALQP) {   // which ones: the first active set of the box QP, whose columns of P all wavefronts form
            if (lane == 0) sFlags[4] = int(unsigned(vm));
        }
    }
    __syncthreads();
    const bool need_qp = sFlags[3] != 0;
    VS_STAMP(5);
    VS_REFRESH_IDS();

#ifdef VS_DIAG_QP   // measurement build: the box QP in four parts -> t_acc[0..3] (see vsmpc_p4.hpp)
    for (int i = 0; i < 4; ++i) t_acc[i] = 0;
    unsigned long long* const qp_cycles = STAMPS ? t_acc : nullptr;
#else
    constexpr unsigned long long* qp_cycles = nullptr;
#endif
    if (need_qp) {
        box_qp<D>(sFlags[3], hold, wave, qp_cycles);
        __syncthreads();
        VS_STAMP(6);
        VS_REFRESH_IDS();
        if constexpr (D::NU % 16 != 0) {
            // joint rows share the first corner tile row with throttle rows: redo the corner sweep with the throttles
            // prescribed (its right-hand side starts over from y)
            init_corner_rhs();
            __syncthreads();
#pragma unroll 1
            for (int p = D::NT - 1; p >= PV; --p) sweep_tile(p, true);
        }
    } else {
        VS_STAMP(6);
    }
    // ---------------------------------------------------------------- P5 joints from the register-resident factor
    switch (wave) {
        case 0:
            if constexpr (PIPE) p5_wave0_jets<D>(smem, lane);
            else backsub_wave<D, TPW, 0, PIPE>(acc, sW, sZ, sXinv, sU, lane);
            break;
        case 1: backsub_wave<D, TPW, 1, PIPE>(acc, sW, sZ, sXinv, sU, lane); break;
        case 2: backsub_wave<D, TPW, 2, PIPE>(acc, sW, sZ, sXinv, sU, lane); break;
        default: backsub_wave<D, TPW, 3, PIPE>(acc, sW, sZ, sXinv, sU, lane); break;
    }
    // (the throttles were final before P5: their copy needs no barrier in front of it; the one behind it also covers the joints)
    if (tid < D::NV) sV[tid] = sZ[D::NU + tid];
    __syncthreads();

    VS_STAMP(7);
    VS_REFRESH_IDS();
    // ---------------------------------------------------------------- P6 forward simulation + outputs
    // the output pointers: requested from the kernarg segment here, a phase ahead of their use (a scalar load is a
    // ~0.5 us round trip when it misses, and nothing else in P6 wants the scalar registers)
#ifdef VS_DIAG_P6   // measurement build: P6 in four pieces -> t_acc[0..3].  Pipelined schedule: the forcing pass / the stream as
                    // wavefront 1 ran it / that wavefront's wait at the closing barrier (what the side work of the other
                    // wavefronts costs) / outputs.  SYRK form: input terms / set-up + first step / other steps / outputs
    for (int i = 0; i < 4; ++i) t_acc[i] = 0;
    VS_TIC();
#define VS_P6_TOC(i) VS_TOC(i)
#else
#define VS_P6_TOC(i) do { } while (0)
#endif
    const SolveArgs* ka = late_args();
    double* xout = ka->xout;
    double* fmout = ka->fmout;
    int* status_out = ka->status_out;
    int* iters_out = ka->iters_out;
    // entry l of the first-move block.  Everything in it is known once the jets' node 1 is; its throttle percentages cost a
    // square root
    auto write_first_move = [&](int l) __attribute__((always_inline)) {
        double v;
        if (l < 8) v = sU[l];                                        // delta q           (variableSamplingMPC.cpp:99)
        else if (l < 12) v = sV[D::NV - 4 + (l - 8)];                // v0                (:100)
        else if (l < 16) v = Jet::throttle_of_v(sV[D::NV - 4 + (l - 12)]);  // throttle % (:146-149)
        else if (l < 20) v = sX[NX + 12 + (l - 16)];                 // thrust, node 1    (:101)
        else v = sX[NX + 16 + (l - 20)];                             // thrust rate, node 1 (:102)
        fmout[size_t(inst) * VSMPC_FM_SIZE + l] = v;
    };
    // wavefront 3 has no element of the input-term pass below (pipelined schedule: 6 N of them): it starts taking the reduced joint
    // unknowns back to joint increments here -- the first three reflectors; the rest beside the first pipeline step
    double u8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    constexpr int JX_SPLIT = PIPE ? 3 : NJC;
    if (PIPE && wave == 3 && lane < D::HC) joint_expand<D, NJC, JX_SPLIT>(smem + S::oQR, sZ + NJC * lane, u8);
    // input terms of every stage in parallel: f_k = Bj U_{jb(k)} + Bt v_{tb(k)} + c  (Bj U = R^T y in the reduced unknowns)
    // (straight-line rounds with clamped indices: the loads of all rounds are in flight together; as a loop with a per-thread
    // trip count the rounds ran one LDS round trip after the other)
    // Pipelined schedule: only the six momentum rows are read from here (the jets formed theirs beside P5, the CoM / RPY link has
    // constant input terms and reads c itself), and every T_k is in sX since P5 (p5_wave0_jets), so the element goes on to the
    // finished forcing g_k = A_mom T_k + f_k.  A seventh element per stage puts -0.0 into row 0: what the lanes of the stream
    // below that have no forcing start their sums from.  7 N elements, one round.
    {
        constexpr int ROWS = PIPE ? 7 : NX;
        constexpr int NE = ROWS * D::N, RND = (NE + D::BLOCK - 1) / D::BLOCK;
        static_assert(!PIPE || RND == 1, "the forcing of the pipelined schedule is one round");
#pragma unroll
        for (int rd = 0; rd < RND; ++rd) {
            const int e0 = tid + rd * D::BLOCK, ec = e0 < NE ? e0 : NE - 1;
            const int k = ec / ROWS, rr = ec - k * ROWS;
            const int r = PIPE ? (rr < 3 ? 3 + rr : (rr < 6 ? 6 + rr : 0)) : rr;   // rows 3..5, 9..11; 0: the -0.0
            const int e = NX * k + r;
            const int jb = joint_block_of_stage<D>(k);
            const int tb = throttle_block_of_stage<D>(k);
            const int vq = tb == 0 ? D::NV - 4 : 4 * (tb - 1);  // internal offset of reference block tb
            double f = sC[r];
#pragma unroll
            for (int c = 0; c < NJC; ++c) f += sBj[r * NJ + c] * sZ[NJC * jb + c];
#pragma unroll
            for (int c = 0; c < NTH; ++c) f += sBt[r * NTH + c] * sV[vq + c];
            if constexpr (PIPE) {
#pragma unroll
                for (int c = 0; c < NTH; ++c) f = fma(sA[r * NX + 12 + c], sX[NX * k + 12 + c], f);
                if (rr == 6) f = -0.0;
            }
            if (e0 < NE) sF[e] = f;
        }
    }
    __syncthreads();
    VS_P6_TOC(0);
    if constexpr (!PIPE) {
        // SYRK form.  The three links of the cascade (jets -> momenta -> CoM / RPY + error integrators; systemDynamicsVSMPC.cpp:
        // 79-103,288-319,384-429) run in THREE wavefronts, one chunk of CHK stages apart: step s = jets of chunk s (wavefront
        // 0), momenta of chunk s - 1 (wavefront 1, after adding A_mom T_k to its forcing), CoM / RPY of chunk s - 2
        // (wavefront 2); a workgroup barrier per step hands the trajectories over through sX.  NCH + 2 steps instead of the
        // 3 NCH chunk-lengths one wavefront needs for the links in series (through v19: 8.1 k cycles at the paper horizon,
        // 17.0 k at the 2x horizon; now 7.1 k / 11.6 k).
        constexpr int CHK = D::N > 20 ? 9 : 6, NCH = (D::N + CHK - 1) / CHK;
        // chain states (registers of the owning lanes, alive across the steps)
        double jT = 0.0, jTd = 0.0, jon = 0.0, ja = 0.0, jb = 0.0;
        double Sk[9], hh[3] = {0.0, 0.0, 0.0};
        double cm0 = 0.0, cm1 = 0.0, cm2 = 0.0, cce = 0.0, cx = 0.0, cee = 0.0;
        const int hr0m = (lane & 1) ? 9 : 3;                       // wavefront 1, lane < 2: h_lin / h_ang
        const int cg = lane / 3, cr = lane - 3 * cg;               // wavefront 2, lane < 6: (half, row)
        const int cxr = (cg ? 6 : 0) + cr, chr0 = cg ? 9 : 3, cer = (cg ? 23 : 20) + cr;
        constexpr int JOFF = 1;   // the momenta run a step behind the jets
        if (wave == 0 && lane < NTH) {
            jon = sA[(12 + lane) * NX + 16 + lane]; ja = sA[(16 + lane) * NX + 12 + lane]; jb = sA[(16 + lane) * NX + 16 + lane];
            jT = sIn[VSMPC_IN_X0 + 12 + lane]; jTd = sIn[VSMPC_IN_X0 + 16 + lane];
            sX[12 + lane] = jT;
            sX[16 + lane] = jTd;
        }
        if (wave == 1 && lane < 2) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                hh[r] = sIn[VSMPC_IN_X0 + hr0m + r];
                sX[hr0m + r] = hh[r];
#pragma unroll
                for (int c = 0; c < 3; ++c) Sk[3 * r + c] = sA[(hr0m + r) * NX + hr0m + c];
            }
        }
        if (wave == 2 && lane < 6) {
            cm0 = sA[cxr * NX + chr0]; cm1 = sA[cxr * NX + chr0 + 1]; cm2 = sA[cxr * NX + chr0 + 2];
            cce = sC[cer];
            cx = sIn[VSMPC_IN_X0 + cxr]; cee = sIn[VSMPC_IN_X0 + cer];
            sX[cxr] = cx;
            sX[cer] = cee;
        }
        // wavefront 3 (no link of the cascade) takes the reduced joint unknowns back to joint increments meanwhile:
        // U_i = W^(-1/2) (Q y_i + N n), one block per lane, into the (dead) partial-sum array of P5
        static_assert(D::NUO <= D::NWAVES * D::NP, "joint increments fit the partial-sum array");
        if (wave == 3 && lane < D::HC) {
            joint_expand<D>(smem + S::oQR, sZ + NJC * lane, u8);
#pragma unroll
            for (int i = 0; i < 8; ++i) sU[NJ * lane + i] = u8[i];
        }
        // ... and sends the input part of the primal on its way to HBM while the cascade runs (the state part follows at the end)
        if (wave == 3 && xout != nullptr) {
            double2* xo = reinterpret_cast<double2*>(xout + size_t(inst) * D::NVAR);  // 16 B per lane stores
            for (int i = lane; i < D::NUO / 2; i += 64) xo[D::NXS / 2 + i] = make_double2(sU[2 * i], sU[2 * i + 1]);
            if (lane < D::NV / 2) {  // reference order v_0..v_{NVB-1}
                const int e = 2 * lane, b = e >> 2, c = e & 3;
                const int q = b == 0 ? D::NV - 4 + c : 4 * (b - 1) + c;
                xo[(D::NXS + D::NUO) / 2 + lane] = make_double2(sV[q], sV[q + 1]);
            }
        }

        static_for<0, NCH + 1 + JOFF>([&](auto scst) __attribute__((always_inline)) {
            constexpr int st = decltype(scst)::value;
            if constexpr (st < NCH) {   // jets, chunk st
                if (wave == 0 && lane < NTH) {
                    constexpr int k0 = st * CHK;
                    double fa[CHK], fb[CHK], dtk[CHK];
#pragma unroll
                    for (int u = 0; u < CHK; ++u) {
                        const int k = (k0 + u < D::N) ? k0 + u : D::N - 1;
                        fa[u] = sF[NX * k + 12 + lane];
                        fb[u] = sF[NX * k + 16 + lane];
                        dtk[u] = sDt[k];
                    }
#pragma unroll
                    for (int u = 0; u < CHK; ++u) {
                        const double dT = fma(jon, jTd, fa[u]);
                        const double dTd = fma(ja, jT, fma(jb, jTd, fb[u]));
                        jT = fma(dtk[u], dT, jT);
                        jTd = fma(dtk[u], dTd, jTd);
                        if (k0 + u < D::N) {
                            sX[NX * (k0 + u + 1) + 12 + lane] = jT;
                            sX[NX * (k0 + u + 1) + 16 + lane] = jTd;
                        }
                    }
                }
            }
            if constexpr (st >= JOFF && st - JOFF < NCH) {   // momenta, chunk st - JOFF
                if (wave == 1) {
                    constexpr int k0 = (st - JOFF) * CHK;
                    constexpr int kn = k0 + CHK < D::N ? CHK : D::N - k0;   // stages of this chunk
                    // forcing g_k = A_mom T_k + f_k on the six momentum rows of the chunk's stages (T_k: the previous step's jets)
                    if (lane < 6 * kn) {
                        const int k = k0 + lane / 6, rr = lane % 6, row = rr < 3 ? 3 + rr : 6 + rr;   // rows 3..5, 9..11
                        double gk = sF[NX * k + row];
#pragma unroll
                        for (int c = 0; c < NTH; ++c) gk = fma(sA[row * NX + 12 + c], sX[NX * k + 12 + c], gk);
                        sF[NX * k + row] = gk;
                    }
                    if (lane < 2) {   // (LDS operations of one wavefront execute in order: the forcing above is visible)
                        double gk[CHK][3], dtk[CHK];
#pragma unroll
                        for (int u = 0; u < CHK; ++u) {
                            const int k = (k0 + u < D::N) ? k0 + u : D::N - 1;
#pragma unroll
                            for (int r = 0; r < 3; ++r) gk[u][r] = sF[NX * k + hr0m + r];
                            dtk[u] = sDt[k];
                        }
#pragma unroll
                        for (int u = 0; u < CHK; ++u) {
                            double dh[3];
#pragma unroll
                            for (int r = 0; r < 3; ++r)
                                dh[r] = fma(Sk[3 * r], hh[0], fma(Sk[3 * r + 1], hh[1], fma(Sk[3 * r + 2], hh[2], gk[u][r])));
#pragma unroll
                            for (int r = 0; r < 3; ++r) hh[r] = fma(dtk[u], dh[r], hh[r]);
                            if (k0 + u < D::N) {
#pragma unroll
                                for (int r = 0; r < 3; ++r) sX[NX * (k0 + u + 1) + hr0m + r] = hh[r];
                            }
                        }
                    }
                }
            }
            if constexpr (st >= JOFF + 1 && st - JOFF - 1 < NCH) {   // CoM / RPY and their error integrators, chunk st - JOFF - 1
                if (wave == 2 && lane < 6) {
                    constexpr int k0 = (st - JOFF - 1) * CHK;
                    double hk[CHK][3], dtk[CHK];
#pragma unroll
                    for (int u = 0; u < CHK; ++u) {
                        const int k = (k0 + u < D::N) ? k0 + u : D::N - 1;
#pragma unroll
                        for (int c = 0; c < 3; ++c) hk[u][c] = sX[NX * k + chr0 + c];
                        dtk[u] = sDt[k];
                    }
#pragma unroll
                    for (int u = 0; u < CHK; ++u) {
                        const double dx = fma(cm0, hk[u][0], fma(cm1, hk[u][1], cm2 * hk[u][2]));
                        cee = fma(dtk[u], cx + cce, cee);
                        cx = fma(dtk[u], dx, cx);
                        if (k0 + u < D::N) {
                            sX[NX * (k0 + u + 1) + cxr] = cx;
                            sX[NX * (k0 + u + 1) + cer] = cee;
                        }
                    }
                }
            }
            if constexpr (st + 1 < NCH + 1 + JOFF) __syncthreads();
            if constexpr (st == 0) VS_P6_TOC(1);
        });
    } else {
        // Pipelined schedule (v37): the momenta link and the CoM / RPY link with its error integrators are ONE lane-parallel
        // stream in wavefront 1, all N stages straight-line, no barrier inside.  One state row per lane, one half of the model per
        // 16-lane row:
        //   16-lane row 0 (linear):   lanes 0..2 h_lin (state rows 3..5),  lanes 3..5 CoM (rows 0..2) + integrators (rows 20..22)
        //   16-lane row 1 (angular):  lanes 0..2 h_ang (rows 9..11),       lanes 3..5 RPY (rows 6..8) + integrators (rows 23..25)
        // Both links multiply a 3 x 3 block by the same h_k, which lanes 0..2 of the row hold: v_fmac_f64 with DPP row_newbcast
        // feeds it to the row inside the FMA, three instructions per stage for both links and both halves.  A momentum lane
        // starts its sum from the forcing g_k, the others from the -0.0 of row 0 of sF: fma(c, h, -0.0) is c * h for every
        // input, signed zeros included, so every operation is the one the three-wavefront cascade did, in its order.
        // The whole wavefront runs the stream under one execution mask (the broadcasts' source lanes must be enabled): lanes
        // without a row have zero coefficients and a zero state, and store into words of their own in the (dead) X region.
        constexpr int JUNK = 128 + NX * (D::N + 1);   // doubles the ownerless stores can reach
        static_assert(JUNK + 2 <= S::NXT * D::TS, "the ownerless stores of the stream stay inside the X region");
        double* junk = sXinv;
#ifdef VS_DIAG_P6
        unsigned long long* p6t = reinterpret_cast<unsigned long long*>(junk + JUNK);   // the stream's start and end (wavefront 1)
#endif
        if (wave == 1) {
#ifdef VS_DIAG_P6
            if constexpr (STAMPS) { if (lane == 0) p6t[0] = __builtin_amdgcn_s_memtime(); }
#endif
            const int half = (lane >> 4) & 1, l = lane & 15;
            const bool own = lane < 32 && l < 6, mom = own && l < 3, integ = own && !mom;
            const int r3 = l < 3 ? l : (l < 6 ? l - 3 : 0);
            const int hc0 = half ? 9 : 3;                                         // first momentum row of the half
            const int srow = (l < 3 ? hc0 : (half ? 6 : 0)) + r3, cer = (half ? 23 : 20) + r3;
            // unconditional loads from addresses that are valid for every lane, selected afterwards
            double c0 = sA[srow * NX + hc0], c1 = sA[srow * NX + hc0 + 1], c2 = sA[srow * NX + hc0 + 2];
            double cce = sC[cer], xs = sIn[VSMPC_IN_X0 + srow], ee = sIn[VSMPC_IN_X0 + cer];
            c0 = own ? c0 : 0.0; c1 = own ? c1 : 0.0; c2 = own ? c2 : 0.0;
            xs = own ? xs : 0.0;
            cce = integ ? cce : 0.0;
            ee = integ ? ee : 0.0;
            double* xp = own ? sX + srow : junk + lane;          // + NX (k + 1): immediate offsets
            double* ep = integ ? sX + cer : junk + 64 + lane;
            const double* gp = sF + (mom ? srow : 0);
            xp[0] = xs;
            ep[0] = ee;
            // at most ~24 stages per batch of loads: the 2x horizon keeps its register picture
            constexpr int NSB = (D::N + 23) / 24, CHS = (D::N + NSB - 1) / NSB;
#pragma unroll
            for (int sb = 0; sb < NSB; ++sb) {
                double gk[CHS], dtk[CHS];
#pragma unroll
                for (int u = 0; u < CHS; ++u) {
                    const int k = (sb * CHS + u < D::N) ? sb * CHS + u : D::N - 1;
                    gk[u] = gp[NX * k];
                    dtk[u] = sDt[k];
                }
#pragma unroll
                for (int u = 0; u < CHS; ++u) {
                    const int k = sb * CHS + u;
                    if (k < D::N) {
                        // The hazard recogniser does not look inside inline assembly: `xs` was written by the previous stage's
                        // last FMA (2 wait states before a DPP read), in front of the first stage possibly under another
                        // execution mask (5).
                        if (k == 0)
                            asm volatile("s_nop 4\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:2 row_mask:0xf bank_mask:0xf" : "+v"(gk[u]) : "v"(xs), "v"(c2));
                        else
                            asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:2 row_mask:0xf bank_mask:0xf" : "+v"(gk[u]) : "v"(xs), "v"(c2));
                        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:1 row_mask:0xf bank_mask:0xf" : "+v"(gk[u]) : "v"(xs), "v"(c1));
                        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf" : "+v"(gk[u]) : "v"(xs), "v"(c0));
                        ee = fma(dtk[u], xs + cce, ee);   // the integrator sees the state of node k
                        xs = fma(dtk[u], gk[u], xs);
                        xp[NX * (k + 1)] = xs;
                        ep[NX * (k + 1)] = ee;
                    }
                }
            }
#ifdef VS_DIAG_P6
            if constexpr (STAMPS) { if (lane == 0) p6t[1] = __builtin_amdgcn_s_memtime(); }
#endif
        }
        // Beside it, none of which may reach the closing barrier behind the stream: wavefront 3 finishes the joint increments
        // U_i = W^(-1/2) (Q y_i + N n), one block per lane, into the (dead) partial-sum array of P5, and sends them and the
        // first-move entries made of them; wavefront 0 sends the throttle part of the primal, wavefront 2 the first-move
        // entries that need no joint (the jets' node 1 is known since P5; their square roots are the long part).
        static_assert(D::NUO <= D::NWAVES * D::NP, "joint increments fit the partial-sum array");
        if (wave == 3) {
            if (lane < D::HC) {
                joint_expand<D, JX_SPLIT, 0>(smem + S::oQR, sZ + NJC * lane, u8);
#pragma unroll
                for (int i = 0; i < 8; ++i) sU[NJ * lane + i] = u8[i];
            }
            if (xout != nullptr) {
                double2* xo = reinterpret_cast<double2*>(xout + size_t(inst) * D::NVAR);  // 16 B per lane stores
                for (int i = lane; i < D::NUO / 2; i += 64) xo[D::NXS / 2 + i] = make_double2(sU[2 * i], sU[2 * i + 1]);
            }
            if (fmout != nullptr && lane < 8) write_first_move(lane);
        }
        if (wave == 0 && xout != nullptr && lane < D::NV / 2) {  // reference order v_0..v_{NVB-1}
            double2* xo = reinterpret_cast<double2*>(xout + size_t(inst) * D::NVAR);
            const int e = 2 * lane, b = e >> 2, c = e & 3;
            const int q = b == 0 ? D::NV - 4 + c : 4 * (b - 1) + c;
            xo[(D::NXS + D::NUO) / 2 + lane] = make_double2(sV[q], sV[q + 1]);
        }
        if (wave == 2 && fmout != nullptr && lane < VSMPC_FM_SIZE - 8) write_first_move(8 + lane);
    }
    __syncthreads();
#ifdef VS_DIAG_P6
    if constexpr (STAMPS && PIPE) {   // the stream and its wait at the closing barrier, as wavefront 1 saw them
        const unsigned long long* p6t = reinterpret_cast<const unsigned long long*>(sXinv + 128 + NX * (D::N + 1));
        const unsigned long long t_now = __builtin_amdgcn_s_memtime();
        t_acc[1] = p6t[1] - p6t[0];
        t_acc[2] = t_now - p6t[1];
        t_mark = t_now;
    } else {
        VS_P6_TOC(2);
    }
#endif
    VS_STAMP(8);
    VS_REFRESH_IDS();

    if (xout != nullptr) {
        double2* xo = reinterpret_cast<double2*>(xout + size_t(inst) * D::NVAR);  // 16 B per lane stores
        for (int i = tid; i < D::NXS / 2; i += D::BLOCK) xo[i] = make_double2(sX[2 * i], sX[2 * i + 1]);
        // (the joint increments and the throttles left from wavefront 3 during the cascade)
    }
    if (!PIPE && fmout != nullptr && tid < VSMPC_FM_SIZE) write_first_move(tid);   // (pipelined schedule: sent during the cascade)
    if (tid == 0) {
        int st = sFlags[1];
        if (sFlags[0]) st = VSMPC_STATUS_NUMERICAL;
        status_out[inst] = st;
        if (iters_out != nullptr) iters_out[inst] = sFlags[2];
    }
    VS_P6_TOC(3);
    VS_STAMP(9);
    if constexpr (STAMPS) {
        unsigned long long* st_ = late_args()->stamps;
        if (tid == 0 && st_ != nullptr) {
#if defined(VS_DIAG_P3) && !defined(VS_DIAG_P6)
            for (int i = 0; i < 4; ++i) t_acc[i] = vs_diag_p3[i];
#endif
            t_acc[5] = __builtin_amdgcn_s_memrealtime() - rt0;
            t_acc[4] = rt0;  // absolute start (global 100 MHz counter): start skew across the workgroups of a launch
            for (int i = 0; i < 6; ++i) st_[size_t(blockIdx.x) * 16 + 10 + i] = t_acc[i];
        }
    }
#undef VS_STAMP
#undef VS_REFRESH_IDS
#undef VS_TIC
#undef VS_TOC
#undef VS_P6_TOC
