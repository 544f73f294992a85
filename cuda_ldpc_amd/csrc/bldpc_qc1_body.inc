// bldpc_qc1_body.inc -- the body of the row kernel, expanded twice by bldpc_qc_kernel.hpp (see bldpc_qc2_body.inc):
//   QC1_NAME k_qc, QC1_PERSIST 0: one workgroup per frame group; QC1_NAME k_qcp, QC1_PERSIST 1: persistent, per-frame exit.
// NORM: normalised min-sum, every check message scaled by a.alpha behind the select of cn_out (see bldpc_qc2_body.inc)
template <typename GM, bool HIST, bool NORM = false> __global__ __launch_bounds__(GM::TPB, GM::MINW) void QC1_NAME(QcArgs a)
{
    constexpr int NF = GM::NF, L = GM::L, Z = GM::Z, WC = GM::WC, WV = GM::WV, G = GM::G;
    constexpr int RPT = GM::RPT, CPT = GM::CPT, MSG = GM::MSG;
    using MT = typename Msg<NF>::T; // one message: the NF frames of a lane side by side (float or v2f32) -- explicit vectors: left
                                    // as scalar floats the compiler paired components of DIFFERENT edges for its packed adds and
                                    // moved them into place (10 v_mov per row pair at J32_L64_Z64)
    constexpr bool LOC = GM::LOC;             // local edges (see QcGeom): slots 0 .. NLR-1 of every row never touch LDS; the thread's
    constexpr int NLR = LOC ? GM::NLR : 0;    // column cc = rr*NLR + pp is the column of local edge pp of its row rr
    static_assert(!LOC || CPT == RPT * GM::NLR, "every column of a thread is the column of one of its local edges");
    constexpr bool USE_PRIO = GM::lds_bytes * 2 <= 160 * 1024; // stage priorities matter between the workgroups that share a CU (see k_qc2)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    // XCD-aware workgroup id: blocks b, b+8, ... share an XCD (and its L2); give each XCD a
    // contiguous range of frames so the 4-byte-per-frame rows of y are fetched into one L2 only.
    const int chunk = (a.nWG + 7) >> 3;
#if QC1_PERSIST
    const int xcd = (int)(blockIdx.x & 7); // persistent workgroups (per-frame exit): frame groups of this XCD from its counter, see k_qc2p
    int wg = 0;
#else
    const int wg = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
    if (wg >= a.nWG) return;
#endif

    const int F = a.F;
    const int tid = threadIdx.x;
    const int g = tid / Z, t = tid - g * Z; // (LOC, whole waves per group: g as a scalar -- table look-ups as scalar loads -- measured: no gain)
#if QC1_PERSIST
    int f0 = 0;
#else
    const int f0 = wg * NF; // first frame of this workgroup
#endif
    int *lds_flag = reinterpret_cast<int *>(lds + GM::flag_byte); // [NF]

    // ---- prologue: rotated slot indices, channel values, zeroed R ----------------------------
    // row j = g + rr*G, block pp:   R slot  (j*WC + pp)*Z + t               (aligned)
    //                               S slot  Sslot + col*Z + (t+s) mod Z     (rotated)
    const int rbase = (g * WC * Z + t) * MSG;          // + (rr*G*WC + pp)*Z*MSG as immediate offsets
    const int sbase = (GM::Sslot + g * Z + t) * MSG;   // + cc*G*Z*MSG
    unsigned saddr[RPT][(WC + 1) / 2];                 // S slots of the row's neighbours, packed 2 x 16 bit
    constexpr bool UNPACKED = RPT * WC <= 16;          // few enough to keep as byte addresses (saves 2 VALU per edge and iteration)
    int saddr_u[UNPACKED ? RPT : 1][UNPACKED ? WC : 1];
    MT Rr[RPT][WC];                                    // this thread's previous outputs R_p: it wrote them, it keeps them (see k_qc2)
    // All table gathers are issued unconditionally (index clamped into the row / column) and only then
    // consumed: predicated loads would be waited for one by one, ~0.4 us each under load.
    int e0v[RPT], wrv[RPT];
#pragma unroll
    for (int rr = 0; rr < RPT; rr++) {
        e0v[rr] = a.rowptr[g + rr * G];
        wrv[rr] = a.rowptr[g + rr * G + 1] - e0v[rr];
    }
    int wcv[CPT]; // LOC: the place of the column's local block among its blocks in ascending block row (scalar: g is wave-uniform)
#pragma unroll
    for (int cc = 0; cc < CPT; cc++) wcv[cc] = LOC ? __builtin_amdgcn_readfirstlane((int)a.wv[g + cc * G]) : (int)a.wv[g + cc * G];
    int sst[LOC ? CPT : 1]; // LOC: byte address of S of this thread's variable of column cc, ((t + shift of the local block) mod Z)
    int cl[LOC ? CPT : 1];  // LOC, prologue only: that circulant position
#pragma unroll
    for (int rr = 0; rr < RPT; rr++) {
        QcCnEdge ed[WC];
#pragma unroll
        for (int pp = 0; pp < WC; pp++) ed[pp] = a.cn_edges[e0v[rr] + min(pp, wrv[rr] - 1)];
#pragma unroll
        for (int pp = 0; pp < WC; pp++) {
            int c = t + ed[pp].shift;
            c = (c >= Z) ? c - Z : c;
            const int slot = (pp < wrv[rr]) ? GM::Sslot + ed[pp].col * Z + c : GM::inf_slot;
            if (pp & 1) saddr[rr][pp / 2] |= (unsigned)slot << 16;
            else saddr[rr][pp / 2] = (unsigned)slot;
            if (UNPACKED) saddr_u[UNPACKED ? rr : 0][UNPACKED ? pp : 0] = slot * MSG;
            if constexpr (LOC) {
                if (pp < NLR) {
                    sst[rr * NLR + pp] = slot * MSG;
                    cl[rr * NLR + pp] = c;
                }
            }
#if !QC1_PERSIST
            const float zero[NF] = {};
            lds_st<NF>(lds, rbase + (rr * G * WC + pp) * Z * MSG, zero); // Memory_RQ = 0 (LDPC_Decoder.cu:82)
            Rr[rr][pp] = MT{};
#endif
        }
    }
    MT yreg[CPT];
    int raddr[CPT][WV]; // byte addresses of the R messages of each variable's edges (LOC: of its WV-1 other edges)
    // channel values of this thread's variable of column cc: one NF*4-byte load per lane (frames >= F were zero-filled by
    // k_regroup_y; the in-place form is only used when every workgroup has NF frames).  LOC: the variable index is its S slot.
    auto y_load = [&](int cc) -> MT {
        const int n = LOC ? sst[LOC ? cc : 0] / MSG - GM::Sslot : (g + cc * G) * Z + t;
        return (NF == 2 && a.y_raw) ? *reinterpret_cast<const MT *>(a.y_raw + (size_t)n * F + f0)
                                    : *reinterpret_cast<const MT *>(a.y + ((size_t)wg * (L * Z) + n) * NF);
    };
#pragma unroll
    for (int cc = 0; cc < CPT; cc++) {
        const int l = g + cc * G; // LOC: a virtual column (the host lists the columns of every row's local blocks)
        if constexpr (LOC) {
            QcVnEdge ed[WV - 1]; // the column's other blocks, ascending block row
#pragma unroll
            for (int k = 0; k < WV - 1; k++) ed[k] = a.vn_edges[l * WV + k];
#if !QC1_PERSIST
            yreg[cc] = y_load(cc);
#endif
#pragma unroll
            for (int k = 0; k < WV - 1; k++) {
                int r = cl[cc] - ed[k].shift;
                r = (r < 0) ? r + Z : r;
                raddr[cc][k] = (ed[k].e * Z + r) * MSG;
            }
        } else {
        QcVnEdge ed[WV];
#pragma unroll
        for (int k = 0; k < WV; k++) ed[k] = a.vn_edges[l * WV + min(k, wcv[cc] - 1)];
#if !QC1_PERSIST
        yreg[cc] = y_load(cc);
#endif
#pragma unroll
        for (int k = 0; k < WV; k++) {
            int r = t - ed[k].shift;
            r = (r < 0) ? r + Z : r;
            raddr[cc][k] = ((k < wcv[cc]) ? ed[k].e * Z + r : GM::zero_slot) * MSG;
        }
        }
    }
    if (tid < NF) {
        reinterpret_cast<float *>(lds)[GM::zero_slot * NF + tid] = 0.0f;
        reinterpret_cast<float *>(lds)[GM::inf_slot * NF + tid] = __builtin_inff();
        lds_flag[tid] = 0;
        lds_flag[NF + tid] = 0;
    }
    unsigned long long hist = 0; // used by threads tid < NF
    unsigned done = 0;           // per-frame exit: frames of this workgroup that have stopped (workgroup-uniform)
    constexpr unsigned ALL = (1u << NF) - 1u;
#ifdef QC_STAMPS
    int nst = 0;
    auto stamp = [&](unsigned long long v) { if (tid == 0 && nst < QC_STAMPS) a.stamps[(size_t)wg * QC_STAMPS + nst++] = v; };
    stamp(((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | __builtin_amdgcn_s_getreg((31 << 11) | 4));
    stamp(__builtin_amdgcn_s_memtime());
#endif
#if !QC1_PERSIST
    __syncthreads();
#endif
#ifdef QC_STAMPS
    stamp(__builtin_amdgcn_s_memtime());
#endif

    // VN phase (LDPC_Decoder.cu:188-210): S = ((0+R_0)+...+R_{w-1})+y, published aligned.
    auto vn_phase = [&](bool (&bad)[NF]) {
        constexpr int CB = (CPT * WV * NF <= 24) ? CPT : ((CPT % 3 == 0) ? 3 : ((CPT % 2 == 0) ? 2 : 1)); // columns with reads in flight together
        static_for<CPT / CB>([&](auto C0) {
            constexpr int c0 = decltype(C0)::value * CB;
            MT R[CB][WV];
#pragma unroll
            for (int ci = 0; ci < CB; ci++)
#pragma unroll
                for (int k = 0; k < WV; k++) R[ci][k] = lds_ldm<NF>(raddr[c0 + ci][k]);
            static_for<CB>([&](auto CI) {
                constexpr int ci = decltype(CI)::value, cc = c0 + ci;
                MT S = MT{};
#pragma unroll
                for (int k = 0; k < WV; k++) S = S + R[ci][k];
                S = S + yreg[cc];
                lds_stm_imm<NF, cc * G * Z * MSG>(sbase, S);
                if (HIST) {
                    const bool in_len = ((g + cc * G) * Z + t) < a.length;
#pragma unroll
                    for (int v = 0; v < NF; v++) bad[v] = bad[v] || (in_len && msg_get<NF>(S, v) < 0);
                }
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the stores above are invisible to the compiler's counters
    };

    // LOC: the same sum with the local block's R from the register that holds it, at its place wcv[cc] in the column's order (a
    // scalar: one of WV straight-line bodies per column); S kept for the check-node phase
    MT Sloc[LOC ? CPT : 1];
    auto vn_phase_loc = [&](bool (&bad)[NF]) {
        if constexpr (LOC) {
        MT R[CPT][WV - 1];
#pragma unroll
        for (int cc = 0; cc < CPT; cc++)
#pragma unroll
            for (int k = 0; k < WV - 1; k++) R[cc][k] = lds_ldm<NF>(raddr[cc][k]);
        static_for<CPT>([&](auto CC) {
            constexpr int cc = decltype(CC)::value, rr = cc / NLR, pp = cc % NLR;
            MT S = MT{};
            static_for<WV>([&](auto KK) {
                constexpr int kk = decltype(KK)::value;
                if (wcv[cc] == kk) {
                    asm volatile("" ::: "memory"); // a real (scalar) branch: left alone the compiler computes all WV sums and selects
                    MT T = MT{};
                    static_for<WV>([&](auto K) {
                        constexpr int k = decltype(K)::value;
                        if constexpr (k == kk) T = T + Rr[rr][pp];
                        else T = T + R[cc][k - (k > kk ? 1 : 0)];
                    });
                    S = T;
                }
            });
            S = S + yreg[cc];
            Sloc[LOC ? cc : 0] = S;
            lds_stm_imm<NF, 0>(sst[LOC ? cc : 0], S);
            if (HIST) {
                const bool in_len = (sst[LOC ? cc : 0] / MSG - GM::Sslot) < a.length;
#pragma unroll
                for (int v = 0; v < NF; v++) bad[v] = bad[v] || (in_len && msg_get<NF>(S, v) < 0);
            }
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    };
    // the same with the places known at compile time (KP = their code, qc_kdigit): the form of the iteration loop -- no branches
    auto vn_phase_kp = [&](auto KP, bool (&bad)[NF]) {
        if constexpr (LOC) {
        constexpr int kp = decltype(KP)::value;
        MT R[CPT][WV - 1];
#pragma unroll
        for (int cc = 0; cc < CPT; cc++)
#pragma unroll
            for (int k = 0; k < WV - 1; k++) R[cc][k] = lds_ldm<NF>(raddr[cc][k]);
        static_for<CPT>([&](auto CC) {
            constexpr int cc = decltype(CC)::value, rr = cc / NLR, pp = cc % NLR, kk = qc_kdigit<WV>(kp, cc);
            MT S = MT{};
            static_for<WV>([&](auto K) {
                constexpr int k = decltype(K)::value;
                if constexpr (k == kk) S = S + Rr[rr][pp];
                else S = S + R[cc][k - (k > kk ? 1 : 0)];
            });
            S = S + yreg[cc];
            Sloc[LOC ? cc : 0] = S;
            lds_stm_imm<NF, 0>(sst[LOC ? cc : 0], S);
            if (HIST) {
                const bool in_len = (sst[LOC ? cc : 0] / MSG - GM::Sslot) < a.length;
#pragma unroll
                for (int v = 0; v < NF; v++) bad[v] = bad[v] || (in_len && msg_get<NF>(S, v) < 0);
            }
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    };
    auto vn_any = [&](bool (&bad)[NF]) {
        if constexpr (LOC) vn_phase_loc(bad);
        else vn_phase(bad);
    };

    // per-iteration flag bookkeeping (LDPC_Decoder.cu:137-147).  Two sets of flag words, used by odd and even
    // iterations in turn: the set read after this iteration's barrier is not written again before the next one, so
    // every thread may read it (per-frame exit) while threads tid < NF clear the other set for the next iteration.
    auto flags_publish = [&](const bool (&bad)[NF], int it) {
#pragma unroll
        for (int v = 0; v < NF; v++)
            if (bad[v]) lds_flag[(it & 1) * NF + v] = 1; // same value from every writer
    };
    auto flags_collect = [&](int it) -> int {
        int flag = 0;
        if (tid < NF) {
            flag = lds_flag[(it & 1) * NF + tid] ? 0 : 1;
            lds_flag[((it + 1) & 1) * NF + tid] = 0;
            if (flag && it <= 64) hist |= (1ull << (it - 1));
        }
        return flag;
    };
    // hard bits (and a-posteriori values) of the frames in `mask`, from the S values this thread has just published
    auto emit = [&](unsigned mask, bool (&bad)[NF]) {
        // opaque copies: keeps the output addresses from being computed ahead of the iteration loop and held (or spilled) through it
        unsigned *obits = a.bits;
        float *oapp = a.app;
        asm volatile("" : "+s"(obits), "+s"(oapp));
#pragma unroll
        for (int cc = 0; cc < CPT; cc++) {
            const int n = (g + cc * G) * Z + t;
            float S[NF];
            lds_ld<NF>(S, lds, sbase + cc * G * Z * MSG); // own value, just written
#pragma unroll
            for (int v = 0; v < NF; v++) {
                if (HIST && !((mask >> v) & 1u)) continue; // workgroup-uniform
                const bool neg = S[v] < 0;
                if (!HIST) bad[v] = bad[v] || (n < a.length && neg);
                // hard bits leave packed, one 32-bit word per half-wave: Z % 32 == 0 keeps the 32 lanes of a
                // half-wave inside one thread group, i.e. on 32 consecutive variables n .. n+31, n % 32 == 0.
                const unsigned long long m = __ballot(neg);
                if ((tid & 31) == 0 && f0 + v < F) obits[(size_t)(f0 + v) * GM::NW + (n >> 5)] = (unsigned)(m >> (tid & 32));
                if (oapp && f0 + v < F) oapp[(size_t)n * F + f0 + v] = S[v];
            }
        }
    };
    // per-frame exit: frames whose flag has just come up leave with this iteration's outputs
    auto retire = [&](int it) -> bool {
        unsigned newly = 0;
#pragma unroll
        for (int v = 0; v < NF; v++)
            if (!lds_flag[(it & 1) * NF + v]) newly |= 1u << v;
        newly &= ~done;
        if (newly) {
            bool unused[NF];
            emit(newly, unused);
            if (tid < NF && ((newly >> tid) & 1u) && f0 + tid < F) a.iters[f0 + tid] = it;
            done |= newly;
        }
        return done == ALL;
    };

    // ---- iterations 1 .. max_iter-1: VN, CN --------------------------------------------------
    // One check row with exactly W edges (W <= WC; W < WC only where the row weight is wave-uniform, i.e. Z is whole waves:
    // J32_L64_Z64 has rows of 5, 6 and 7 edges).  Rows lighter than W read the +inf slot in their padding positions.
    auto s_load = [&](int rr, int pp) -> MT {
        if (UNPACKED) return lds_ldm<NF>(saddr_u[UNPACKED ? rr : 0][UNPACKED ? pp : 0]);
        return lds_ldm<NF>((int)((pp & 1) ? (saddr[rr][pp / 2] >> 16) : (saddr[rr][pp / 2] & 0xffffu)) * MSG);
    };
    // All of a thread's check rows with W slots each (W <= WC; W < WC only where the rows, hence their weights, are wave-uniform,
    // i.e. Z is whole waves: J32_L64_Z64 has rows of 5, 6 and 7 edges, paired by weight on the host).  The S values of every row
    // are requested before the first row's arithmetic: with one workgroup per CU nobody else fills a load's latency.  Slots beyond
    // a row's own weight read the +inf slot.
    auto cn_rows = [&](auto WW) {
        constexpr int W = decltype(WW)::value;
        MT Sv[RPT][W];
#pragma unroll
        for (int rr = 0; rr < RPT; rr++)
#pragma unroll
            for (int pp = 0; pp < W; pp++) {
                if (LOC && pp < NLR) Sv[rr][pp] = Sloc[LOC ? rr * NLR + pp : 0]; // the thread's own variable: S from its register
                else Sv[rr][pp] = s_load(rr, pp);
            }
        static_for<RPT>([&](auto RR) {
            constexpr int rr = decltype(RR)::value;
#pragma unroll
            for (int pp = 0; pp < W; pp++) Rr[rr][pp] = Sv[rr][pp] - Rr[rr][pp]; // Q = S - R  (LDPC_Decoder.cu:206-209), in place of R_p
            float m2[NF];
            uint32_t key[NF];
#pragma unroll
            for (int v = 0; v < NF; v++) {
                CnAcc acc;
                cn_two_smallest<W, NF>(reinterpret_cast<const float *>(&Rr[rr][0]) + v, acc.m1, acc.m2, acc.sgn);
                m2[v] = acc.m2;
                key[v] = acc.key();
            }
            if (USE_PRIO) __builtin_amdgcn_s_setprio(QC_PRIO_WR);
            static_for<W>([&](auto PP) {
                constexpr int pp = decltype(PP)::value;
                MT Rn;
#pragma unroll
                for (int v = 0; v < NF; v++) msg_set<NF>(Rn, v, cn_out(msg_get<NF>(Rr[rr][pp], v), m2[v], key[v]));
                if constexpr (NORM) Rn = Rn * a.alpha;
                Rr[rr][pp] = Rn;
                if constexpr (!(LOC && pp < NLR)) lds_stm_imm<NF, (rr * G * WC + pp) * Z * MSG>(rbase, Rn); // a local edge's R has no reader but this thread
            });
            if (USE_PRIO) __builtin_amdgcn_s_setprio(QC_PRIO_CN);
        });
    };
#if QC1_PERSIST
    for (;;) { // frame groups of this workgroup
    if (tid == 0) lds_flag[0] = atomicAdd(&a.work[xcd], 1); // (a flag word carries it: no static __shared__ object, the dynamic segment starts at 0)
    __syncthreads();
    {
        const int ord = __builtin_amdgcn_readfirstlane(lds_flag[0]);
        if (ord >= chunk || xcd * chunk + ord >= a.nWG) break;
        wg = xcd * chunk + ord;
    }
    __syncthreads(); // everybody has the group before the flag words are reset
    f0 = wg * NF;
#pragma unroll
    for (int rr = 0; rr < RPT; rr++)
#pragma unroll
        for (int pp = 0; pp < WC; pp++) {
            const float zero[NF] = {};
            lds_st<NF>(lds, rbase + (rr * G * WC + pp) * Z * MSG, zero); // Memory_RQ = 0 (LDPC_Decoder.cu:82)
            Rr[rr][pp] = MT{};
        }
#pragma unroll
    for (int cc = 0; cc < CPT; cc++) yreg[cc] = y_load(cc);
    if (tid < NF) {
        lds_flag[tid] = 0;
        lds_flag[NF + tid] = 0;
    }
    hist = 0;
    done = 0;
    __syncthreads();
#endif
    // The iteration loop, one instantiation per row weight W: where the rows of a thread are wave-uniform (ROWU) the scalar choice of
    // the body is made ONCE, outside the loop -- made per iteration the three bodies left their new R_p in different registers and
    // the loop's back edge carried 22 v_mov per wave and iteration to bring them together.
    auto iterate = [&](auto WW, auto KP) {
    for (int it = 1; it < a.max_iter; it++) {
        // keep the 16-bit-packed slot indices packed across iterations (unpacked they cost 2x the VGPRs)
#pragma unroll
        for (int rr = 0; rr < RPT; rr++)
#pragma unroll
            for (int i = 0; i < (WC + 1) / 2; i++)
                if (!UNPACKED) asm volatile("" : "+v"(saddr[rr][i]));
        bool bad[NF];
#pragma unroll
        for (int v = 0; v < NF; v++) bad[v] = false;
        if (USE_PRIO) __builtin_amdgcn_s_setprio(QC_PRIO_VN);
        if constexpr (LOC) {
            if constexpr (decltype(KP)::value >= 0) vn_phase_kp(KP, bad);
            else vn_phase_loc(bad); // (places read at run time, a branch per column)
        } else vn_phase(bad);
        if (HIST) flags_publish(bad, it);
#ifdef QC_STAMPS
        if (it == 20 && tid == 0) a.stamps[(size_t)wg * QC_STAMPS + 120] = __builtin_amdgcn_s_memtime(); // wave 0 reaches the VN barrier
#endif
        __syncthreads();
#ifdef QC_STAMPS
        stamp(__builtin_amdgcn_s_memtime());
#endif
        if (USE_PRIO) __builtin_amdgcn_s_setprio(QC_PRIO_CN);
        if (HIST) {
            (void)flags_collect(it);
            if (a.per_frame && retire(it)) return;
        }

        // CN phase (LDPC_Decoder.cu:279-314)
        cn_rows(WW);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#ifdef QC_STAMPS
        if (it == 20 && tid == 0) a.stamps[(size_t)wg * QC_STAMPS + 121] = __builtin_amdgcn_s_memtime(); // wave 0 reaches the CN barrier
#endif
        __syncthreads();
#ifdef QC_STAMPS
        stamp(__builtin_amdgcn_s_memtime());
#endif
    }
    };
    // LOC: the code of the thread group's places (a scalar), and one loop per sorted code: the host orders blocks and rows so that no
    // other occurs (a code that is not sorted would mean tables of another build: the wave then runs the branching form below)
    int kcode = 0;
    if constexpr (LOC) {
#pragma unroll
        for (int cc = CPT - 1; cc >= 0; cc--) kcode = kcode * WV + wcv[cc];
    }
    auto iterate_w = [&](auto WW) {
        if constexpr (LOC && HIST) {
            iterate(WW, std::integral_constant<int, -1>{}); // the flag-tracking instantiation (batch-global rule, histories) keeps the one branching loop: 66 loops there are 210 KB of code
        } else if constexpr (LOC) {
            constexpr int NCODE = qc_ipow(WV, CPT);
            bool ran = false;
            static_for<NCODE>([&](auto C) {
                if constexpr (qc_kcode_sorted<WV, RPT, (LOC ? NLR : 1)>(decltype(C)::value)) {
                    if (kcode == decltype(C)::value) {
                        iterate(WW, C);
                        ran = true;
                    }
                }
            });
            if (!ran) iterate(WW, std::integral_constant<int, -1>{});
        } else {
            iterate(WW, std::integral_constant<int, 0>{});
        }
    };
    {
        constexpr bool ROWU = (Z % 64 == 0) && WC >= 4; // rows, hence their weights, are wave-uniform: a scalar branch picks the body
        if constexpr (ROWU) {
            int wu = 0;
#pragma unroll
            for (int rr = 0; rr < RPT; rr++) wu = max(wu, __builtin_amdgcn_readfirstlane(wrv[rr]));
            if (wu <= WC - 2) iterate_w(std::integral_constant<int, WC - 2>{});
            else if (wu == WC - 1) iterate_w(std::integral_constant<int, WC - 1>{});
            else iterate_w(std::integral_constant<int, WC>{});
        } else {
            iterate_w(std::integral_constant<int, WC>{});
        }
    }

    // ---- final iteration: VN only (the CN pass after it is unobservable), then outputs -----------
    int flag = 0;
    if (!(HIST && done == ALL)) {
        bool bad[NF];
#pragma unroll
        for (int v = 0; v < NF; v++) bad[v] = false;
        vn_any(bad);
        if (LOC) __syncthreads(); // emit reads S in the natural layout: other threads' stores
        emit(~done, bad);
        flags_publish(bad, a.max_iter);
        __syncthreads();
        flag = flags_collect(a.max_iter);
    }
#ifdef QC_STAMPS
    stamp(__builtin_amdgcn_s_memtime());
#endif
    if (tid < NF && f0 + tid < F) {
        const bool stopped = HIST && ((done >> tid) & 1u);
        a.D[(size_t)L * Z * F + f0 + tid] = stopped ? 1 : flag;
        if (HIST && a.hist) a.hist[f0 + tid] = hist;
        if (HIST && a.per_frame && !stopped) a.iters[f0 + tid] = a.max_iter;
    }
#if QC1_PERSIST
    __syncthreads(); // everybody is done with this group's S and flags before the next group's state goes in
    } // next frame group
#endif
}
