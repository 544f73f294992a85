// bldpc_qc2_body.inc -- the body of the half-row kernel, expanded twice by bldpc_qc_kernel.hpp:
//   QC2_NAME k_qc2,  QC2_PERSIST 0: one workgroup per frame pair (every exit mode);
//   QC2_NAME k_qc2p, QC2_PERSIST 1: PERSISTENT workgroups for the per-frame exit -- frames leave after 1 ... max_iter iterations, and
//       dispatched one workgroup per pair the CUs end far apart (as the GF(q) kernels did, DESIGN 6): the grid fills the chip once
//       and a workgroup takes pair after pair of its XCD from a counter; tables and rotated addresses are set up once.
// GM::LOC selects the local-edge form (QcGeom2), in both expansions.
// NORM: normalised min-sum (bldpc_decode_normalised).  The clamp-XOR select of cn_out maps (m1, m2) to (m2, m1) and cannot map them to
// (alpha m2, alpha m1), so its result is scaled: fl(alpha * (+-m)) has the bits of +-fl(alpha * m), one v_pk_mul_f32 per edge and frame pair.
template <typename GM, bool HIST, bool NORM = false> __global__ __launch_bounds__(GM::TPB, GM::MINW) void QC2_NAME(QcArgs a)
{
    constexpr int NF = GM::NF, L = GM::L, Z = GM::Z, WC = GM::WC, WV = GM::WV, GJ = GM::GJ, ZB = GM::ZB, WCH = GM::WCH;
    constexpr int RPT = GM::RPT, CPT = GM::CPT, NCG = GM::NCG, MSG = GM::MSG;
    static_assert(NF == 2, "the half-row kernel carries a frame pair per lane");
    constexpr bool LOC = GM::LOC;       // local edges, see QcGeom2: edges 0 .. NL-1 of a half-row never touch LDS
    constexpr int NL = LOC ? CPT : 0;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int chunk = (a.nWG + 7) >> 3; // XCD-aware workgroup id, see k_qc
#if QC2_PERSIST
    // persistent workgroups (per-frame exit only, see the end of this file's user): XCD x = blockIdx & 7 owns the frame pairs
    // [x chunk, (x+1) chunk) and its workgroups take them one after the other from the XCD's counter a.work[x]
    const int xcd = (int)(blockIdx.x & 7);
    int wg = 0;
#else
    const int wg = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
    if (wg >= a.nWG) return;
#endif

    const int F = a.F;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, h = lane >> 5;
    const int jq = wave / ZB, t = (wave - jq * ZB) * 32 + (lane & 31);
    const int cg = jq * 2 + h;  // column group of this half-wave
#if QC2_PERSIST
    int f0 = 0;
#else
    const int f0 = wg * NF;
#endif
    int *lds_flag = reinterpret_cast<int *>(lds + GM::flag_byte);

    // row j = jq + rr*GJ, this thread's edges pp = h*WCH + i
    const int rbase = ((jq * WC + h * WCH) * Z + t) * MSG;   // + (rr*GJ*WC + i)*Z*MSG
    const int sbase = (GM::Sslot + cg * Z + t) * MSG;        // + cc*NCG*Z*MSG
    int saddr[RPT][WCH]; // byte addresses of the S values of this thread's edges
    v2f32 Rr[RPT][WCH];  // this thread's previous outputs R_p (+0 at the start, Memory_RQ = 0, LDPC_Decoder.cu:82: see vn_first)
    int sst[LOC ? CPT : 1];   // LOC: byte address of S of this thread's variable of column cc, (t + shift of the local block) mod Z
    int raddr[CPT][WV];       // byte addresses of the R values the variable-node phase reads (LOC: the WV-1 other block rows)
    {   // every address from the host's table (QcPlan::d_lane): one coalesced load, nothing gathered here
        constexpr int NV = LOC ? CPT : 0, WVR = LOC ? WV - 1 : WV;
        int w[4 * GM::LW];
#pragma unroll
        for (int k = 0; k < GM::LW; k++) {
            const v4i32 x = a.lane[k * GM::TPB + tid];
            w[4 * k] = x.x; w[4 * k + 1] = x.y; w[4 * k + 2] = x.z; w[4 * k + 3] = x.w;
        }
#pragma unroll
        for (int cc = 0; cc < NV; cc++) sst[LOC ? cc : 0] = (GM::Sslot + w[cc]) * MSG;
#pragma unroll
        for (int rr = 0; rr < RPT; rr++)
#pragma unroll
            for (int i = 0; i < WCH; i++) saddr[rr][i] = w[NV + rr * WCH + i];
#pragma unroll
        for (int cc = 0; cc < CPT; cc++)
#pragma unroll
            for (int k = 0; k < WVR; k++) raddr[cc][k] = w[NV + RPT * WCH + cc * WVR + k];
    }
    v2f32 yreg[CPT];
    // channel values of this thread's variable of column cc (LOC: variable index = its S slot)
    auto y_load = [&](int cc) -> v2f32 {
        const int n = LOC ? sst[LOC ? cc : 0] / MSG - GM::Sslot : (cg + cc * NCG) * Z + t;
        return a.y_raw ? *reinterpret_cast<const v2f32 *>(a.y_raw + (size_t)n * F + f0)
                       : *reinterpret_cast<const v2f32 *>(a.y + ((size_t)wg * (L * Z) + n) * NF);
    };
#if !QC2_PERSIST
#pragma unroll
    for (int cc = 0; cc < CPT; cc++) yreg[cc] = y_load(cc);
#endif
    if (tid < NF) {
        reinterpret_cast<float *>(lds)[GM::zero_slot * NF + tid] = 0.0f;
        reinterpret_cast<float *>(lds)[GM::inf_slot * NF + tid] = __builtin_inff();
        lds_flag[tid] = 0;
        lds_flag[NF + tid] = 0;
    }
    unsigned long long hist = 0;
    unsigned done = 0; // per-frame exit, see k_qc
    constexpr unsigned ALL = (1u << NF) - 1u;
#ifdef QC_STAMPS
    int nst = 0;
    auto stamp = [&](unsigned long long v) { if (tid == 0 && nst < QC_STAMPS) a.stamps[(size_t)wg * QC_STAMPS + nst++] = v; };
    const unsigned hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    stamp(((unsigned long long)xcc << 32) | hwid);
    stamp(__builtin_amdgcn_s_memtime());
    if (a.stagger && ((hwid >> 16) & 1))
        for (int i = 0; i < a.stagger; i += 64 * 16) __builtin_amdgcn_s_sleep(16);
#endif
#if !QC2_PERSIST
    __syncthreads();
#endif
#ifdef QC_STAMPS
    stamp(__builtin_amdgcn_s_memtime());
#endif

    // VN phase (LDPC_Decoder.cu:188-210): S = ((0+R_0)+...+R_{w-1})+y, published aligned.  0 + R_0 is a real addition:
    // R_0 may be -0.0f (magnitude 0, sign -1) and (+0) + (-0) = +0 is what the reference computes.
    // ZS (compile time) = the sum starts at 0; without it it starts at R_0, one v_pk_add_f32 per column less.  The two forms differ
    // only where EVERY addend is -0.0f, y included: the reference's sum is +0.0f there, the short one -0.0f.  Then this variable's R
    // is -0.0f on every edge, so the check-node phase's Q = S - R is +0.0f both ways, and S < 0 is false both ways; a column with an
    // absent block row adds the +0.0f slot and never gets there.  What does read the sign of a zero S is emit (app and its bits).
    // So the short form is for sums that only the next check-node phase reads: the iteration loop of the HIST == false
    // instantiations, where emit runs after the FINAL variable-node phase only, and that one (vn_any) keeps the 0.  With HIST,
    // retire emits S from inside the loop (per-frame exit, k_qc2p) and every phase keeps it.  vn_first is exact as it stands.
    auto vn_phase = [&](auto ZS, bool (&bad)[NF]) {
        constexpr bool zs = decltype(ZS)::value;
        constexpr int CB = (CPT * WV <= 12) ? CPT : 1; // columns with reads in flight together
        static_for<CPT / CB>([&](auto C0) {
            constexpr int c0 = decltype(C0)::value * CB;
            v2f32 R[CB][WV];
#pragma unroll
            for (int ci = 0; ci < CB; ci++)
#pragma unroll
                for (int k = 0; k < WV; k++) R[ci][k] = lds_ld2(raddr[c0 + ci][k]);
            static_for<CB>([&](auto CI) {
                constexpr int ci = decltype(CI)::value, cc = c0 + ci;
                v2f32 S = R[ci][0];
                if constexpr (zs) S = v2f32{0.0f, 0.0f} + S;
#pragma unroll
                for (int k = 1; k < WV; k++) S = S + R[ci][k];
                S = S + yreg[cc];
                lds_st2_imm<cc * NCG * Z * MSG>(sbase, S);
                if (HIST) {
                    const bool in_len = ((cg + cc * NCG) * Z + t) < a.length;
                    bad[0] = bad[0] || (in_len && S.x < 0);
                    bad[1] = bad[1] || (in_len && S.y < 0);
                }
            });
            if (CB < CPT) __builtin_amdgcn_sched_barrier(0);
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the stores above are invisible to the compiler's counters
    };
    // LOC: the same sum with the own block row's R from the register that holds it (slot jj), S kept for the check-node phase
    v2f32 Sloc[LOC ? CPT : 1];
    const int jqs = __builtin_amdgcn_readfirstlane(jq);
    auto vn_phase_loc = [&](auto JJ, auto ZS, bool (&bad)[NF], auto &&pre_wait) {
        constexpr int jj = decltype(JJ)::value;
        constexpr bool zs = decltype(ZS)::value;
        v2f32 R[CPT][WV - 1];
#pragma unroll
        for (int cc = 0; cc < CPT; cc++)
#pragma unroll
            for (int kk = 0; kk < WV - 1; kk++) R[cc][kk] = lds_ld2(raddr[cc][kk]);
        static_for<CPT>([&](auto CC) {
            constexpr int cc = decltype(CC)::value;
            v2f32 S = v2f32{0.0f, 0.0f};
            static_for<WV>([&](auto K) {
                constexpr int k = decltype(K)::value;
                v2f32 Rk;
                if constexpr (k == jj) Rk = Rr[0][cc];
                else Rk = R[cc][k - (k > jj ? 1 : 0)];
                if constexpr (k == 0 && !zs) S = Rk;
                else S = S + Rk;
            });
            S = S + yreg[cc];
            Sloc[LOC ? cc : 0] = S;
            lds_st2_imm<0>(sst[LOC ? cc : 0], S);
            if (HIST) {
                const bool in_len = (sst[LOC ? cc : 0] / MSG - GM::Sslot) < a.length;
                bad[0] = bad[0] || (in_len && S.x < 0);
                bad[1] = bad[1] || (in_len && S.y < 0);
            }
        });
        pre_wait();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    // The first variable-node phase: every R is +0 (Memory_RQ = 0, LDPC_Decoder.cu:82), so the reference's sum ((0+R_0)+...+R_{w-1})+y
    // is (+0) + y = y + 0.0f bit for bit (y = -0.0f included): no R is read, none had to be zeroed in LDS.
    auto vn_first = [&](bool (&bad)[NF], auto &&pre_wait) {
        static_for<CPT>([&](auto CC) {
            constexpr int cc = decltype(CC)::value;
            const v2f32 S = yreg[cc] + v2f32{0.0f, 0.0f};
            int n;
            if constexpr (LOC) {
                Sloc[LOC ? cc : 0] = S;
                lds_st2_imm<0>(sst[LOC ? cc : 0], S);
                n = sst[LOC ? cc : 0] / MSG - GM::Sslot;
            } else {
                lds_st2_imm<cc * NCG * Z * MSG>(sbase, S);
                n = (cg + cc * NCG) * Z + t;
            }
            if (HIST) {
                const bool in_len = n < a.length;
                bad[0] = bad[0] || (in_len && S.x < 0);
                bad[1] = bad[1] || (in_len && S.y < 0);
            }
        });
        pre_wait();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    auto no_early = []() {};
    auto vn_any = [&](bool (&bad)[NF]) {
        if constexpr (LOC) static_for<GM::J>([&](auto JJ) { if (jqs == decltype(JJ)::value) vn_phase_loc(JJ, std::true_type{}, bad, no_early); });
        else vn_phase(std::true_type{}, bad);
    };
    auto flags_publish = [&](const bool (&bad)[NF], int it) { // two sets of flag words by iteration parity, see k_qc
#pragma unroll
        for (int v = 0; v < NF; v++)
            if (bad[v]) lds_flag[(it & 1) * NF + v] = 1;
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
    auto emit = [&](unsigned mask, bool (&bad)[NF]) {
        unsigned *obits = a.bits; // opaque copies, see k_qc
        float *oapp = a.app;
        asm volatile("" : "+s"(obits), "+s"(oapp));
#pragma unroll
        for (int cc = 0; cc < CPT; cc++) {
            const int n = (cg + cc * NCG) * Z + t;
            float S[NF];
            lds_ld<NF>(S, lds, sbase + cc * NCG * Z * MSG);
#pragma unroll
            for (int v = 0; v < NF; v++) {
                if (HIST && !((mask >> v) & 1u)) continue; // workgroup-uniform
                const bool neg = S[v] < 0;
                if (!HIST) bad[v] = bad[v] || (n < a.length && neg);
                const unsigned long long m = __ballot(neg); // one 32-bit word per half-wave, see k_qc
                if ((tid & 31) == 0 && f0 + v < F) obits[(size_t)(f0 + v) * GM::NW + (n >> 5)] = (unsigned)(m >> (tid & 32));
                if (oapp && f0 + v < F) oapp[(size_t)n * F + f0 + v] = S[v];
            }
        }
    };
    auto retire = [&](int it) -> bool { // per-frame exit, see k_qc
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

#if QC2_PERSIST
    for (;;) { // frame pairs of this workgroup
    if (tid == 0) lds_flag[0] = atomicAdd(&a.work[xcd], 1); // (a flag word carries it: no static __shared__ object, the dynamic segment starts at 0)
    __syncthreads();
    {
        const int ord = __builtin_amdgcn_readfirstlane(lds_flag[0]);
        if (ord >= chunk || xcd * chunk + ord >= a.nWG) break;
        wg = xcd * chunk + ord;
    }
    __syncthreads(); // everybody has the pair before the flag words are reset
    f0 = wg * NF;
    // this pair's state: its channel values, no flags (every R = +0: the first iteration reads none, see vn_first)
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
    // Scheduling of the local edges (DESIGN 4.1).  The first triple of a half-row's selection network is its local edges (NL >= 3): their
    // Q = Sloc - R, the triple's lo / mid and the XOR of its sign words need no LDS access.  cn_local computes them between the last S
    // store of the variable-node phase and its drain wait, where the wave would stand idle, instead of behind the S reads of the
    // check-node phase: 14.62 -> 15.00 M codewords/s (the same work between the issue of the S reads and their first wait: 14.68;
    // profiles/r08_qc2_local_sched_ab.txt).  Q replaces R_p in Rr[0][0 .. NL-1] here already.  Only an iteration does this: the final
    // variable-node phase (vn_any) needs R_p as the last check-node phase left it.  Where retire leaves between the barrier and the
    // check-node phase the early values are unused: the pair is done, and the next pair's first iteration overwrites them.
    constexpr int NE = (NL >= 3 && WCH >= 4) ? 3 : 0; // edges handled ahead: the first triple
    float elo[NF], emid[NF];
    uint32_t esg[NF];
    auto cn_local = [&](auto FIRST) {
        constexpr bool first = decltype(FIRST)::value;
#pragma unroll
        for (int i = 0; i < NL; i++) Rr[0][i] = first ? Sloc[LOC ? i : 0] : Sloc[LOC ? i : 0] - Rr[0][i];
#pragma unroll
        for (int v = 0; v < NF; v++) cn_lead_triple<2>(reinterpret_cast<const float *>(&Rr[0][0]) + v, elo[v], emid[v], esg[v]);
    };
    // Iteration it (1 ... max_iter-1): variable-node phase, barrier, check-node phase, barrier.  FIRST (it = 1): every R is +0, the
    // variable-node phase is vn_first and the check-node phase's Q = S - R is Q = S (S - (+0) == S for every S, -0.0f included).
    // True when the per-frame exit has retired every frame of the pair.
    auto iteration = [&](auto JJ, auto FIRST, int it) -> bool {
        constexpr bool first = decltype(FIRST)::value;
        bool bad[NF];
#pragma unroll
        for (int v = 0; v < NF; v++) bad[v] = false;
        __builtin_amdgcn_s_setprio(QC_PRIO_VN);
        auto early = [&]() { // between the phase's last S store and its drain wait
            if constexpr (NE > 0) {
                cn_local(FIRST);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if constexpr (first) vn_first(bad, early);
        else if constexpr (LOC) vn_phase_loc(JJ, std::bool_constant<HIST>{}, bad, early); // the loop's sums: from 0 only where emit may read them
        else vn_phase(std::bool_constant<HIST>{}, bad);
        if (HIST) flags_publish(bad, it);
        __syncthreads();
        __builtin_amdgcn_s_setprio(QC_PRIO_CN);
#ifdef QC_STAMPS
        stamp(__builtin_amdgcn_s_memtime());
#endif
        if (HIST) {
            (void)flags_collect(it);
            if (a.per_frame && retire(it)) return true;
        }

        // CN phase (LDPC_Decoder.cu:279-314)
#pragma unroll
        for (int rr = 0; rr < RPT; rr++) {
            CnAcc acc[NF];
            {   // in two batches: every load in flight holds a register pair, and 6 waves per SIMD leave 80 registers per lane
                // (LOC: the half-row's 7 remaining S reads go out together -- 14 registers, which the local edges freed: 12.18 -> 12.56 M
                // codewords/s, profiles/r03_qc2_variants.txt)
#ifdef QC2_CHK_SPLIT /* experiment: two batches also with local edges */
                constexpr int CHK = (WCH > 6) ? (WCH + 1) / 2 : WCH;
#else
                constexpr int CHK = (WCH > 6 && !LOC) ? (WCH + 1) / 2 : WCH;
#endif
#pragma unroll
                for (int c0 = 0; c0 < WCH; c0 += CHK) {
                    v2f32 Sv[CHK];
#pragma unroll
                    for (int i = 0; i < CHK && c0 + i < WCH; i++) {
                        if (LOC && c0 + i < NL) Sv[i] = Sloc[LOC ? c0 + i : 0]; // the thread's own variable: S from its register
                        else Sv[i] = lds_ld2(saddr[rr][c0 + i]);
                    }
#pragma unroll
                    for (int i = 0; i < CHK && c0 + i < WCH; i++)
                        if (!(NE > 0 && c0 + i < NL)) Rr[rr][c0 + i] = first ? Sv[i] : Sv[i] - Rr[rr][c0 + i]; // Q = S - R  (LDPC_Decoder.cu:206-209), in place of R_p
                    if (c0 + CHK < WCH) __builtin_amdgcn_sched_barrier(0);
                }
            }
#if QC_ACC_RUNNING
            static_assert(NE == 0, "the running accumulator takes every edge");
#pragma unroll
            for (int v = 0; v < NF; v++) acc[v].init();
#pragma unroll
            for (int i = 0; i < WCH; i++) {
                acc[0].add(Rr[rr][i].x);
                acc[1].add(Rr[rr][i].y);
            }
#else
            if constexpr (NE > 0) {
#pragma unroll
                for (int v = 0; v < NF; v++)
                    cn_two_smallest_lead<WCH, 2>(elo[v], emid[v], esg[v], reinterpret_cast<const float *>(&Rr[rr][NE]) + v, acc[v].m1, acc[v].m2, acc[v].sgn);
            } else {
                cn_two_smallest<WCH, 2>(reinterpret_cast<const float *>(&Rr[rr][0]), acc[0].m1, acc[0].m2, acc[0].sgn);
                cn_two_smallest<WCH, 2>(reinterpret_cast<const float *>(&Rr[rr][0]) + 1, acc[1].m1, acc[1].m2, acc[1].sgn);
            }
#endif
            // merge the two halves of the row: the two smallest of {m1,m2} U {m1',m2'}, XOR of the signs
            uint32_t a1 = f2u(acc[0].m1), b1 = f2u(acc[1].m1), a2 = f2u(acc[0].m2), b2 = f2u(acc[1].m2), as = acc[0].sgn, bs = acc[1].sgn;
            swap32(a1, b1); // lanes 0-31: (own, other half's) value of frame 0; lanes 32-63: (other half's, own) value of frame 1
            swap32(a2, b2);
            swap32(as, bs);
            const uint32_t m1 = min(a1, b1);
            uint32_t m2u = min(min(max(a1, b1), a2), b2);
            uint32_t keyu = __builtin_amdgcn_bitop3_b32(m1, m2u, __builtin_amdgcn_bitop3_b32(as, bs, 0x80000000u, 0x28), 0x96); // (m1 ^ m2) ^ ((as ^ bs) & sign)
            uint32_t m2v = m2u, keyv = keyu;
            swap32(m2u, m2v);   // m2u: frame 0 (computed by lanes 0-31), m2v: frame 1, in every lane
            swap32(keyu, keyv);
            const float m2f[NF] = {u2f(m2u), u2f(m2v)};
            const uint32_t key[NF] = {keyu, keyv};
            __builtin_amdgcn_s_setprio(LOC ? QC_PRIO_WR_LOC : QC_PRIO_WR);
            static_for<RPT * WCH>([&](auto I) {
                constexpr int r_ = decltype(I)::value / WCH, i = (decltype(I)::value % WCH + NL) % WCH; // the stored edges first
                if (r_ != rr) return;
                v2f32 Rn;
                Rn.x = cn_out(Rr[rr][i].x, m2f[0], key[0]);
                Rn.y = cn_out(Rr[rr][i].y, m2f[1], key[1]);
                if constexpr (NORM) Rn = Rn * a.alpha;
                Rr[rr][i] = Rn;
                if constexpr (!(LOC && i < NL)) lds_st2_imm<(r_ * GJ * WC + i) * Z * MSG>(rbase, Rn); // a local edge's R has no reader but this thread
            });
        }
        // the local edges' outputs have no store: they stand between the last store and the drain wait, not behind it where the last wave to
        // reach the barrier spent them after idling (14.39 -> 14.62 M codewords/s; one local edge after every second store: the same)
        if (NL > 0) __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
#ifdef QC_STAMPS
        stamp(__builtin_amdgcn_s_memtime());
#endif
        return false;
    };
    // The first iteration on its own straight-line path, then the loop; LOC: one instantiation of the loop per block row JJ of the wave,
    // chosen ONCE outside it (chosen per iteration the J sums left S in different registers and the back edge carried three v_mov_b64
    // per wave and iteration, see k_qc)
    const bool retired = a.max_iter > 1 && iteration(std::integral_constant<int, 0>{}, std::true_type{}, 1);
    auto iterate = [&](auto JJ) {
        for (int it = 2; it < a.max_iter; it++)
            if (iteration(JJ, std::false_type{}, it)) return;
    };
    if (!retired) {
        if constexpr (LOC) static_for<GM::J>([&](auto JJ) { if (jqs == decltype(JJ)::value) iterate(JJ); });
        else iterate(std::integral_constant<int, 0>{});
    }

    int flag = 0;
    if (!(HIST && done == ALL)) { // final iteration: VN only, then outputs
        bool bad[NF];
#pragma unroll
        for (int v = 0; v < NF; v++) bad[v] = false;
        if (a.max_iter > 1) vn_any(bad);
        else vn_first(bad, no_early);
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
#if QC2_PERSIST
    __syncthreads(); // everybody is done with this pair's S and flags before the next pair's state goes in
    } // next frame pair
#endif
}

