// Dual step, device helpers: the float64 MFMA contractions over the columns of the staged bundle (Gram matrix of the rank test,
// H | A z of a Newton update).  Included by be_dual_dev.h; everything is in an anonymous namespace.
#pragma once
#include "be_dual_cut.h"

namespace icnn_be {

namespace {

// D = A B^T style contractions over the columns of the LDS bundle with f64 MFMA.
//   HESS = false:  Hm[i][j] = sum_c A[i][c] A[j][c]                     (Gram, rank test)
//   HESS = true :  Hm[i][j] = sum_c A[i][c] w[c] A[j][c]   (j < k)       dual :36
//                  Hm[i][k] = sum_c A[i][c] z[c]                         dual :35
// A operand: lane (r16, q) holds A[ti*16+r16][c0+q]; B operand: lane holds B[c0+q][tj*16+r16].
// Result: lane holds D[ti*16 + q + 4r][tj*16 + r16], r = 0..3 (f64 C/D map).
// Small bundles (at most 8 rows/columns of output): v_mfma_f64_4x4x4_4b_f64, whose four 4x4 blocks
// are used as the 2x2 tiling of an 8x8 result.  Measured lane layout on gfx950
// (tools/probes/mfma_f64_4x4_probe.hip): with kq = lane>>4, block = (lane>>2)&3, r = lane&3
//   A operand lane holds A_block[r][kq], B operand lane holds B_block[kq][r],
//   result lane holds D_block[lane>>4][lane&3].
// Same 4 columns per instruction as the 16x16x4 form, but 4 passes instead of 16.
// Operand masking without arithmetic: the bundle in LDS is followed by a row of zeros (row `zrow`) and
// a row of ones (row `zrow + 1`).  A lane whose output row/column is outside the bundle reads the zero
// row; the lane that produces column k (A z) reads the ones row and z instead of a bundle row and w.
// So per k-step a lane converts two cut values and does one multiply -- same bits as masking with 0/1
// factors (x * 1 = x, fma(x, w, +-0) = x * w).
struct NoLap { __device__ void operator()(int) const {} };
template <typename CutT, bool HESS, typename LapF = NoLap>
__device__ void contract_mfma_8x8(const CutT *As, int ldA, int k, const CutT *crow, int cbeg, int cend,
                                  const double *ws, const double *zs, double *Hm, int HP, LapF lapf = LapF()) {
    const int lane = thread_id() & 63, kq = lane >> 4, blk = (lane >> 2) & 3, r = lane & 3;
    const int ra = 4 * (blk >> 1) + r, cb = 4 * (blk & 1) + r;
    const bool zcol = HESS && cb == k;
    // crow: the constant rows -- zeros at crow[0 .. ldA), ones at crow[ldA .. 2 ldA)
    const CutT *pa = (ra < k ? As + ra * ldA : crow) + kq;
    const CutT *pb = (cb < k ? As + cb * ldA : (zcol ? crow + ldA : crow)) + kq;
    const double *pwz = (zcol ? zs : ws) + kq;
    double acc0 = 0.0, acc1 = 0.0;                       // two chains hide the MFMA latency
    cbeg = uni(cbeg); cend = uni(cend);                  // scalar loop control
    // Software pipeline, distance one: the LDS reads of the next 16 columns are issued before the four
    // MFMAs of the current 16, so the LDS round trip overlaps the arithmetic instead of preceding it.
    // Two register sets alternate (no copies); scheduling barriers and an opaque use after the MFMAs
    // keep the compiler from folding the prefetch back into "load, wait, use".
    CutT xa[4], xb[4], ya[4], yb[4];
    double xw[4], yw[4];
    auto gather = [&](int c0, CutT (&ga)[4], CutT (&gb)[4], double (&gw)[4]) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            ga[s] = pa[c0 + 4 * s];
            gb[s] = pb[c0 + 4 * s];
            if (HESS) gw[s] = pwz[c0 + 4 * s];
        }
    };
    auto stage = [&](int cnext, CutT (&ca)[4], CutT (&cb_)[4], double (&cw)[4], CutT (&na)[4], CutT (&nb)[4],
                     double (&nw)[4]) {
        gather(cnext, na, nb, nw);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double av = (double)ca[s];
            const double bv = HESS ? (double)cb_[s] * cw[s] : (double)cb_[s];
            if (s & 1) acc1 = __builtin_amdgcn_mfma_f64_4x4x4f64(av, bv, acc1, 0, 0, 0);
            else acc0 = __builtin_amdgcn_mfma_f64_4x4x4f64(av, bv, acc0, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; ++s) { pin(na[s]); pin(nb[s]); if (HESS) pin(nw[s]); }
    };
    if (cbeg < cend) gather(cbeg, xa, xb, xw);
    // Nothing may be outstanding when the loop is entered: otherwise the wait-count pass, merging the
    // preheader state into the loop header, puts an lgkmcnt(0) right behind the prefetch of every stage.
    __builtin_amdgcn_s_waitcnt(0xc07f);                  // lgkmcnt(0), visible to the wait-count pass
    lapf(10);
    const int clast = cend - 16;
    for (int c0 = cbeg; c0 < cend; c0 += 32) {           // column range is a multiple of 16
        stage(c0 + 16 < cend ? c0 + 16 : clast, xa, xb, xw, ya, yb, yw);
        if (c0 + 16 < cend) stage(c0 + 32 < cend ? c0 + 32 : clast, ya, yb, yw, xa, xb, xw);
    }
    lapf(11);
    const int row = 4 * (blk >> 1) + kq, col = 4 * (blk & 1) + r;
    const int ncolsB = HESS ? k + 1 : k;
    if (row < k && col < ncolsB) Hm[row * HP + col] = acc0 + acc1;
}

// 17 .. 20 cuts (round 6): TWO 16 x 16 tiles instead of the three of the (ti, tj) tiling below, whose tiles (0, 1) and (1, 1)
// hold 1 .. 5 useful columns each.  A tile's A-operand rows and B-operand columns need not be contiguous -- every lane picks its
// row pointer --, so the pairs that involve the extra rows e = 16 .. k - 1 fit ONE tile:
//   tile 1   rows 0 .. 15  x  columns 0 .. 14 and A z (HESS) / 0 .. 15 (Gram);  H[i][15] = H[15][i] by symmetry (HESS)
//   tile 2   rows 4 .. 19  x  columns { 16 .. 19,  A z,  0 .. 3,  15 }: (i, e) for i = 4 .. 19, (A z)_e, (e, i) for i = 0 .. 3
//            mirrored into (i, e), and the diagonal entry (15, 15) that tile 1 gave up for A z.
// A float64 16x16x4 MFMA occupies the wave for ~125 cycles with its operand set-up (tools/probes/dual_update_probe.hip: 5.0 k
// cycles per tile sweep of 160 columns), so a Newton update at 17 .. 20 cuts drops from 15 k to 10 k cycles here, the rank
// test's Gram matrix from 13.6 k to 9.4 k.  Same k-ordered fma chains per entry; the entries (i, 15), i < 15, and (i, e), i < 4,
// are now formed with the OTHER factor carrying the weight w (H is symmetric: they differ from the three-tile result in the
// last bit).  Every kernel takes this path for such bundles, so the dispatch paths stay bit-identical among themselves.
template <typename CutT, bool HESS>
__device__ void contract_mfma_cover2(const CutT *As, int ldA, int k, const CutT *crow, int cbeg, int cend, const double *ws,
                                     const double *zs, double *Hm, int HP) {
    const int lane = thread_id() & 63, r16 = lane & 15, q = lane >> 4;
    cbeg = uni(cbeg); cend = uni(cend);
    constexpr int ZC = 64, NONE = 65;                          // B-operand column codes besides a bundle row
#pragma unroll 1
    for (int t = 0; t < 2; ++t) {
        const int ra = t == 0 ? r16 : 4 + r16;                 // A-operand row of this lane
        int cb;                                                // B-operand column of this lane
        if (t == 0) cb = HESS ? (r16 < 15 ? r16 : ZC) : r16;
        else if (r16 < 4) cb = 16 + r16;
        else if (HESS) cb = r16 == 4 ? ZC : (r16 < 9 ? r16 - 5 : (r16 == 9 ? 15 : NONE));
        else cb = r16 < 8 ? r16 - 4 : NONE;
        const bool zcol = cb == ZC;
        const CutT *pa = (ra < k ? As + ra * ldA : crow) + q;
        const CutT *pb = (cb < k ? As + cb * ldA : (zcol ? crow + ldA : crow)) + q;
        const double *pwz = (zcol ? zs : ws) + q;
        d4 acc = {0.0, 0.0, 0.0, 0.0}, acc_odd = {0.0, 0.0, 0.0, 0.0};
        CutT xa[4], xb[4], ya[4], yb[4];                       // software pipeline as in contract_mfma_8x8
        double xw[4], yw[4];
        auto gather = [&](int c0, CutT (&ga)[4], CutT (&gb)[4], double (&gw)[4]) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                ga[s] = pa[c0 + 4 * s];
                gb[s] = pb[c0 + 4 * s];
                if (HESS) gw[s] = pwz[c0 + 4 * s];
            }
        };
        auto stage = [&](int cnext, CutT (&ca)[4], CutT (&cb_)[4], double (&cw)[4], CutT (&na)[4], CutT (&nb)[4], double (&nw)[4]) {
            gather(cnext, na, nb, nw);
            __builtin_amdgcn_sched_barrier(0);
            // all four operand chains (cvt, cvt, mul) FIRST, then the four MFMAs back to back: float64 VALU work issued while
            // the wave's own float64 MFMA is in flight stalls on the shared DP pipe -- interleaved, an MFMA with its chain costs
            // a lone wave 204 cycles, batched 115 (the MFMA alone: 70; tools/probes/mfma_overlap_probe.hip).  Same arithmetic.
            double av[4], bv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                av[s] = (double)ca[s];
                bv[s] = HESS ? (double)cb_[s] * cw[s] : (double)cb_[s];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (s & 1) acc_odd = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc_odd, 0, 0, 0);
                else acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 4; ++s) { pin(na[s]); pin(nb[s]); if (HESS) pin(nw[s]); }
        };
        if (cbeg < cend) gather(cbeg, xa, xb, xw);
        __builtin_amdgcn_s_waitcnt(0xc07f);                    // lgkmcnt(0), see contract_mfma_8x8
        const int clast = cend - 16;
        for (int c0 = cbeg; c0 < cend; c0 += 32) {             // column range is a multiple of 16
            stage(c0 + 16 < cend ? c0 + 16 : clast, xa, xb, xw, ya, yb, yw);
            if (c0 + 16 < cend) stage(c0 + 32 < cend ? c0 + 32 : clast, ya, yb, yw, xa, xb, xw);
        }
        acc += acc_odd;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (t == 0 ? 0 : 4) + q + 4 * r;      // bundle row of this result
            if (row >= k) continue;
            if (zcol) {
                if (t == 0 || row >= 16) Hm[row * HP + k] = acc[r];
            } else if (t == 0) {
                Hm[row * HP + cb] = acc[r];                                        // (rows 0 .. 15) x (columns 0 .. 14 | 15)
                if (HESS && row == 15) Hm[cb * HP + 15] = acc[r];                  // H[i][15] = H[15][i]
            } else if (cb < k) {
                if (cb >= 16) {                                                    // (i, e), i = 4 .. 19
                    Hm[row * HP + cb] = acc[r];
                    if (row < 16) Hm[cb * HP + row] = acc[r];
                } else if (cb < 4) {                                               // (e, i), i = 0 .. 3, and its mirror
                    if (row >= 16) { Hm[row * HP + cb] = acc[r]; Hm[cb * HP + row] = acc[r]; }
                } else if (row == 15) {                                            // cb == 15: the diagonal entry
                    Hm[15 * HP + 15] = acc[r];
                }
            }
        }
    }
}

template <typename CutT, int KT, bool HESS, typename LapF = NoLap>
__device__ void contract_mfma(const CutT *As, int ldA, int k, const CutT *crow, int cbeg, int cend, const double *ws,
                              const double *zs, double *Hm, int HP, LapF lapf = LapF()) {
    const int lane = thread_id() & 63, r16 = lane & 15, q = lane >> 4;
    const int ncolsB = HESS ? k + 1 : k;
    if (ncolsB <= 8) {
        contract_mfma_8x8<CutT, HESS>(As, ldA, k, crow, cbeg, cend, ws, zs, Hm, HP, lapf);
        return;
    }
    if (KT > 16 && k >= 17 && k <= 20) {
        contract_mfma_cover2<CutT, HESS>(As, ldA, k, crow, cbeg, cend, ws, zs, Hm, HP);
        return;
    }
    cbeg = uni(cbeg); cend = uni(cend);
    for (int ti = 0; ti * 16 < k; ++ti) {
        for (int tj = ti; tj * 16 < ncolsB; ++tj) {
            d4 acc = {0.0, 0.0, 0.0, 0.0}, acc_odd = {0.0, 0.0, 0.0, 0.0};   // two chains: a dependent
            const int ra = ti * 16 + r16, cb = tj * 16 + r16;              // 16x16x4 f64 MFMA costs 65 cycles
            const bool zcol = HESS && cb == k;
            const CutT *pa = (ra < k ? As + ra * ldA : crow) + q;
            const CutT *pb = (cb < k ? As + cb * ldA : (zcol ? crow + ldA : crow)) + q;
            const double *pwz = (zcol ? zs : ws) + q;
            CutT xa[4], xb[4], ya[4], yb[4];                    // software pipeline as in contract_mfma_8x8
            double xw[4], yw[4];
            auto gather = [&](int c0, CutT (&ga)[4], CutT (&gb)[4], double (&gw)[4]) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    ga[s] = pa[c0 + 4 * s];
                    gb[s] = pb[c0 + 4 * s];
                    if (HESS) gw[s] = pwz[c0 + 4 * s];
                }
            };
            auto stage = [&](int cnext, CutT (&ca)[4], CutT (&cb_)[4], double (&cw)[4], CutT (&na)[4],
                             CutT (&nb)[4], double (&nw)[4]) {
                gather(cnext, na, nb, nw);
                __builtin_amdgcn_sched_barrier(0);
                // (round 6: the four operand chains first, then the MFMAs back to back -- see contract_mfma_cover2)
                double av[4], bv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    av[s] = (double)ca[s];
                    bv[s] = HESS ? (double)cb_[s] * cw[s] : (double)cb_[s];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    // (only in the 32-slot kernels, whose bundles actually live here: the 16-slot kernel is held
                    //  to 128 VGPRs and the second accumulator would spill in its Newton loop)
                    if (KT > 16 && (s & 1)) acc_odd = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc_odd, 0, 0, 0);
                    else acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 4; ++s) { pin(na[s]); pin(nb[s]); if (HESS) pin(nw[s]); }
            };
            if (cbeg < cend) gather(cbeg, xa, xb, xw);
            __builtin_amdgcn_s_waitcnt(0xc07f);                 // lgkmcnt(0), see contract_mfma_8x8
            const int clast = cend - 16;
            for (int c0 = cbeg; c0 < cend; c0 += 32) {          // column range is a multiple of 16
                stage(c0 + 16 < cend ? c0 + 16 : clast, xa, xb, xw, ya, yb, yw);
                if (c0 + 16 < cend) stage(c0 + 32 < cend ? c0 + 32 : clast, ya, yb, yw, xa, xb, xw);
            }
            if (KT > 16) acc += acc_odd;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = ti * 16 + q + 4 * r, col = tj * 16 + r16;
                if (row < k && col < ncolsB) {
                    Hm[row * HP + col] = acc[r];
                    if (tj != ti && col < k) Hm[col * HP + row] = acc[r];
                }
            }
        }
    }
}

}  // namespace
}  // namespace icnn_be
