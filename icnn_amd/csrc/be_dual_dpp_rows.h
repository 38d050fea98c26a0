// The DPP row algebra of the dual step -- unpivoted LDL^T inertia and the reduced Newton solve for systems of up to 16 rows --
// as text that be_dual_solve.h includes twice (inside its namespaces; no include guard):
//   DPP_ROWS_ATTR = __noinline__,    DPP_ROWS_NAME(f) = f         the functions every dual body calls
//   DPP_ROWS_ATTR = __forceinline__, DPP_ROWS_NAME(f) = f##_inl   the same code inlined: the capped bodies (DualCfg::KCAP > 0)
// Two definitions from one text, so that the called functions keep the tokens (and the machine code) they always had.
template <int KS>
__device__ DPP_ROWS_ATTR int DPP_ROWS_NAME(inertia_not_above_dpp)(const double *Hm_, int HP, int k, double mu) {
    static_assert(KS <= 16, "row broadcasts stay inside one 16-lane row");
    const int lane = lane_id();
    lds_cdouble *Hm = (lds_cdouble *)Hm_;
    HP = uni(HP); k = uni(k); mu = uni(mu);
    double M[KS];
#pragma unroll
    for (int j = 0; j < KS; ++j) M[j] = Hm[(lane < k ? lane : 0) * HP + (j < k ? j : 0)];
#pragma unroll
    for (int j = 0; j < KS; ++j) pin(M[j]);                       // unconditional loads, all in flight
#pragma unroll
    for (int j = 0; j < KS; ++j)
        M[j] = (lane < k && j < k) ? M[j] - (j == lane ? mu : 0.0) : (j == lane ? 1.0 : 0.0);
    double dp = 1.0;                                              // lane p keeps pivot p
    static_for<0, KS>([&](auto P) {
        constexpr int p = decltype(P)::value;
        const double d = row_bcast<p>(M[p]);
        dp = lane == p ? d : dp;
        const double nf = lane > p ? -(M[p] * rcp_nr(d)) : 0.0;
        static_for<p + 1, KS>([&](auto J) {
            constexpr int j = decltype(J)::value;
            M[j] = __builtin_fma(nf, row_bcast<p>(M[j]), M[j]);
        });
    });
    // pivots up to the first exact zero count individually; behind it everything counts as suspect
    const unsigned long long nonpos = __ballot(lane < k && !(dp > 0.0));
    const unsigned long long zero = __ballot(lane < k && dp == 0.0);
    if (zero) {
        const int p0 = __builtin_ctzll(zero);
        return __popcll(nonpos & ((2ull << p0) - 1ull)) + (k - p0 - 1);
    }
    return __popcll(nonpos);
}

// TRI: the system is read from the packed upper triangle the fused VALU pass leaves for a one-wave sample -- entry (r, c),
// r <= c, at c (c + 1) / 2 + r (be_dual_valu_dev.h) -- instead of from a k x (k + 1) matrix: no gather of the sums into a matrix
// in front of every Newton update, three index operations per entry here.  Same values, same elimination.
template <int KS, bool TRI = false>
__device__ DPP_ROWS_ATTR StepResult DPP_ROWS_NAME(newton_step_dpp)(const double *Hm_, int HP, int k, int piv,
                                                                  unsigned long long fmask, bool is_free, double g0) {
    static_assert(KS <= 16, "row broadcasts stay inside one 16-lane row");
    const int lane = lane_id();
    lds_cdouble *Hm = (lds_cdouble *)Hm_;
    HP = uni(HP); k = uni(k); piv = uni(piv); fmask = uni(fmask);
    double M[KS + 1];
    const int rl = lane < k ? lane : 0;
    auto at = [&](int i, int j) -> int {                 // where H[i][j] lives
        if (!TRI) return i * HP + j;
        const int c = i > j ? i : j, r = i > j ? j : i;
        return c * (c + 1) / 2 + r;
    };
    double h_ip = Hm[at(rl, piv)], h_pp = Hm[at(piv, piv)];
#pragma unroll
    for (int j = 0; j < KS; ++j) M[j] = Hm[at(rl, j < k ? j : 0)];
    pin(h_ip);
    pin(h_pp);
#pragma unroll
    for (int j = 0; j < KS; ++j) pin(M[j]);                       // all loads in flight, none sunk into a branch
    // H0[i][j] = ((H[i][j] - keep_i H[j][piv]) - H[i][piv] keep_j) + H[piv][piv] keep_i keep_j, where H[j][piv]
    // is what lane j holds as its own H[.][piv]: one row broadcast instead of a second LDS read (and no second
    // register array -- this function's register need is what the caller has to spill around the call)
    static_for<0, KS>([&](auto J) {
        constexpr int j = decltype(J)::value;
        double hv = ((M[j] - row_bcast<j>(h_ip)) - h_ip) + h_pp;
        pin(hv);                                                  // plain select below, no exec-mask branch
        const bool use = j < k && is_free && ((fmask >> j) & 1ull);
        M[j] = use ? hv : (j == lane ? 1.0 : 0.0);
    });
    M[KS] = is_free ? -g0 : 0.0;
    double rinv = 1.0;                                            // lane p keeps 1 / pivot p
    bool bad = false;
    static_for<0, KS>([&](auto P) {
        constexpr int p = decltype(P)::value;
        const double d = row_bcast<p>(M[p]);
        bad |= !(d != 0.0);                                       // exact zero (or NaN): singular for LAPACK
        const double inv = rcp_nr(d);
        rinv = lane == p ? inv : rinv;
        const double nf = lane > p ? -(M[p] * inv) : 0.0;
        static_for<p + 1, KS + 1>([&](auto J) {
            constexpr int j = decltype(J)::value;
            M[j] = __builtin_fma(nf, row_bcast<p>(M[j]), M[j]);
        });
        __builtin_amdgcn_sched_barrier(0);     // keep the broadcasts of later pivots from being hoisted (registers)
    });
    if (__ballot(bad) & 0xffffull) return StepResult{0.0, 0};
    static_for<0, KS>([&](auto Q) {
        constexpr int p = KS - 1 - decltype(Q)::value;
        const double x = row_bcast<p>(M[KS] * rinv);
        M[KS] = lane == p ? x : (lane < p ? __builtin_fma(-M[p], x, M[KS]) : M[KS]);
    });
    return StepResult{is_free ? M[KS] : 0.0, 1};
}
