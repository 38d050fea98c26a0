// Device code of the FC-PICNN energy/gradient (included by be_picnn_fc.hip and be_fused.hip).
#pragma once
// Fused forward + y-gradient of the y-dependent part of a fully-connected PICNN.
//
//   z_i = act( (z_{i-1} * gate_i) Wzu_i + (y * yu_i) Wyu_i + zu_i ),  i = 0..L,  E = z_L
//   (multi-label-cls/icnn_ebundle.py:349-388, RL/src/icnn.py:356-404) and
//   dE/dy = sum_i yu_i * (delta_i Wyu_i^T),  delta_{i-1} = gate_i * (delta_i Wzu_i^T) * act'(.)
//   (what tf.gradients(E_, y_) evaluates, icnn_ebundle.py:146).
//
// One workgroup owns a tile of TM = 16 samples (one MFMA M-tile; 8 or 4 for a model whose 16-row tile outgrows the LDS:
// icnn_be_fc_model.tile_rows, FcGeom.lds_rows) for the whole chain: the
// activations never leave LDS, the x-only context (yu, zu, gate) is read once per layer with
// coalesced loads, and the non-negative W^(z) / unconstrained W^(y) weights are streamed from
// L2/HBM exactly once per workgroup per pass as pre-packed v_mfma_f32_16x16x4_f32 B-fragments
// (16 B per lane, 1 KiB per wave-instruction).  Each wave owns a strided set of 16-column
// output tiles.  fp32 throughout, like the reference's TensorFlow graph.
#include <hip/hip_runtime.h>

#include "be_common.h"
#include "be_kernels.h"
#include "icnn_be.h"

namespace icnn_be {

namespace {

constexpr int TM = 16;     // samples per workgroup
constexpr int NWAVE = 16;  // waves per workgroup
constexpr int NTHREADS = NWAVE * 64;

__host__ __device__ constexpr int pad16(int v) { return (v + 15) & ~15; }

// The deal of one evaluation (fc_deal below): which wave runs which moved unit in which barrier interval.  Part of the geometry.
struct FcDeal {
    int bwd_moved;                                     // dE/dy_i runs in the interval of layer i - 1, dE/dy_0 ends behind the last barrier
    unsigned short dy_mask[ICNN_BE_MAX_LAYERS][NWAVE]; // [i][w]: the tiles of dE/dy_i on wave w (bwd_moved)
    unsigned short e_mask[NWAVE];                      // [w]: the energy rows of wave w
};

struct FcArgs {
    int n, L;                              // L = number of hidden z-layers (n_layers - 1)
    int width[ICNN_BE_MAX_LAYERS];
    float alpha;
    int action_box;
    int ctx_width;
    int yu_off[ICNN_BE_MAX_LAYERS], zu_off[ICNN_BE_MAX_LAYERS], gate_off[ICNN_BE_MAX_LAYERS];
    long long w_yu_f[ICNN_BE_MAX_LAYERS], w_yu_b[ICNN_BE_MAX_LAYERS];   // float offsets into wpack
    long long w_zu_f[ICNN_BE_MAX_LAYERS], w_zu_b[ICNN_BE_MAX_LAYERS];
    int zb_off[ICNN_BE_MAX_LAYERS], zb_ld[ICNN_BE_MAX_LAYERS];          // LDS float offsets / pitches
    int ldY, ybuf_off, aop_off[ICNN_BE_MAX_LAYERS], gbuf_off, dl_off, lds_floats;   // aop_i = y * yu_i
    int lds_rows;                          // rows every LDS buffer holds: TM, or the model's narrow tile (8, 4); >= tile_rows
    FcDeal deal;
    const float *wpack, *ctx;
    const double *y;
    float *f, *g;
    const int *finished;
    int batch;
    int tile_rows;      // samples a workgroup's 16-row MFMA tile actually holds (lds_rows; 4 or 8 when the batch has fewer
                        // than a full tile per CU: be_fused.hip) -- the other rows are zero
    long long *prof;    // diagnostic: [workgroup][wave][FC_PROF_PHASES] cycle counters, else nullptr
};
constexpr int FC_PROF_PHASES = 16;

// PF: the k-blocks of every packed operand are padded (zero fragments) to a multiple of it -- the unroll factor and ring
// size of the per-sample kernel's fma chains (gemv_chain, be_picnn_fc_rows_dev.h), whose body then needs no bounds checks.
// TILE_RD: depth of the B-fragment register ring (= unroll factor) of the MFMA tile loops.  Measured on one box, whole
// evaluation: depth 5 over the padded k-blocks 124.5 k cycles, depth 2 over the padded k-blocks the same, depth 2 over the
// real k-blocks (38 instead of 40 for K = 600) 118.5 k, depth 1 147 k, depth 10 (one-tile loops) 125.6 k.
constexpr int PF = 5;
constexpr int TILE_RD = 2;
// TILE_PAIR: a wave takes its tiles nt, nt + NWAVE as a pair that shares every A fragment read from LDS (two-tile loop of
// gemm_loop) instead of one after the other.  Off: on one box 1.036 against 1.042 ms for the headline solve -- the LDS reads
// were never the bound -- with eight accumulator and ring registers fewer in the 128-register kernels.
constexpr bool TILE_PAIR = false;
constexpr int TILE_STEP = (TILE_PAIR ? 2 : 1) * NWAVE;
__host__ __device__ constexpr int kblocks(int K) { return (pad16(K) / 16 + PF - 1) / PF * PF; }
// k-blocks the MFMA tile loops of fc_fg_tile walk: the real ones, up to a multiple of their ring depth (the pack's further
// zero fragments would add nothing: acc + 0 * a == acc bit for bit, acc is never -0)
// (an odd number of real k-blocks that IS the pack's -- 5, 15, 25: widths 65-80, 225-240, ... -- has no zero fragment to round
// up into; gemm_tiles runs their last k-block behind the loop)
__host__ __device__ constexpr int kblocks_tile(int K) {
    const int up = (pad16(K) / 16 + TILE_RD - 1) / TILE_RD * TILE_RD;
    return up <= kblocks(K) ? up : kblocks(K);
}

// LDS row pitch (floats): multiple of 4 and == 8 (mod 64) so that the ds_read_b128 A-fragment gather
// (16 rows x 4 k-quads) is bank-conflict free, and wide enough for every k-block the GEMM
// loops read (the padded ones included).
__host__ __device__ constexpr int lds_pitch(int width) {
    int p = kblocks(width) * 16;
    while ((p & 63) != 8) p += 4;
    return p;
}

// floats of one packed GEMM operand W[K][N]
constexpr size_t packed_floats(int K, int N) { return (size_t)kblocks(K) * (pad16(N) / 16) * 256; }

// pack[(kb*NT + nt)*256 + lane*4 + s] = W[kb*16 + 4*(lane>>4) + s][nt*16 + (lane&15)]
// `transpose`: the logical operand is src^T (src stored [N][K] row-major).
// k-block major: at any moment the eight waves of a workgroup (each on its own output tiles, all at about
// the same k-block) read neighbouring 1 KiB fragments, i.e. one contiguous 8-16 KiB window that spreads
// over all L2 channels.  With the tile-major order used at first, the sixteen concurrent streams were
// 10 or 38 KiB apart and marched through the same few channels in lockstep: 13 B/clk per CU instead of
// the ~55 B/clk a workgroup can pull from L2 (tools/probes/l2_stream_probe.hip).
void pack_operand(const float *src, int K, int N, bool transpose, float *dst) {
    const int KB = kblocks(K), NT = pad16(N) / 16;
    for (int nt = 0; nt < NT; ++nt)
        for (int kb = 0; kb < KB; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 4; ++s) {
                    const int kk = kb * 16 + 4 * (lane >> 4) + s, nn = nt * 16 + (lane & 15);
                    float v = 0.f;
                    if (kk < K && nn < N) v = transpose ? src[(size_t)nn * K + kk] : src[(size_t)kk * N + nn];
                    dst[((size_t)(kb * NT + nt) * 64 + lane) * 4 + s] = v;
                }
}

struct PackOffsets {
    long long yu_f[ICNN_BE_MAX_LAYERS], yu_b[ICNN_BE_MAX_LAYERS], zu_f[ICNN_BE_MAX_LAYERS],
        zu_b[ICNN_BE_MAX_LAYERS];
    size_t total;
};
constexpr PackOffsets pack_offsets(int n, int n_layers, const int *width) {
    PackOffsets o{};
    size_t at = 0;
    const int L = n_layers - 1;
    for (int i = 0; i <= L; ++i) {
        const int wi = width[i];
        if (i < L) {
            o.yu_f[i] = (long long)at; at += packed_floats(n, wi);
            o.yu_b[i] = (long long)at; at += packed_floats(wi, n);
            if (i > 0) {
                o.zu_f[i] = (long long)at; at += packed_floats(width[i - 1], wi);
                o.zu_b[i] = (long long)at; at += packed_floats(wi, width[i - 1]);
            }
        } else {   // final scalar layer: plain vectors, 16-float aligned
            o.yu_f[i] = o.yu_b[i] = (long long)at; at += (size_t)pad16(n);
            o.zu_f[i] = o.zu_b[i] = (long long)at; at += (size_t)pad16(width[i - 1]);
        }
    }
    o.total = at;
    return o;
}
inline PackOffsets pack_offsets(const icnn_be_fc_model &m) { return pack_offsets(m.n, m.n_layers, m.width); }

// The geometry of a model: everything fc_fg_tile needs that follows from n and the widths alone.  ONE walk (fc_geom) yields it
// for both shape policies (be_kernels.h): fill_args copies it into the FcArgs of a launch, FixedShape keeps it as a constant.
// The field names are FcArgs' own, so that the device code reads either through the same expressions.
struct FcGeom {
    int n, L;
    int width[ICNN_BE_MAX_LAYERS];
    int ctx_width;
    int yu_off[ICNN_BE_MAX_LAYERS], zu_off[ICNN_BE_MAX_LAYERS], gate_off[ICNN_BE_MAX_LAYERS];
    long long w_yu_f[ICNN_BE_MAX_LAYERS], w_yu_b[ICNN_BE_MAX_LAYERS];
    long long w_zu_f[ICNN_BE_MAX_LAYERS], w_zu_b[ICNN_BE_MAX_LAYERS];
    int zb_off[ICNN_BE_MAX_LAYERS], zb_ld[ICNN_BE_MAX_LAYERS];
    int ldY, ybuf_off, aop_off[ICNN_BE_MAX_LAYERS], gbuf_off, dl_off, lds_floats;
    int lds_rows;
    FcDeal deal;
};

// ---- the deal -------------------------------------------------------------------------------------------------------------
// An evaluation is 2 L barrier intervals: forward layers 0 .. L-1 (intervals 0 .. L-1), backward layers L-1 .. 0 (intervals
// L .. 2L-1), and what runs behind the last barrier (interval 2L).  Its units, each one 16-column output tile of one GEMM:
//   FC_UNIT_FWD_Y  (y * yu_i) Wyu_i             FC_UNIT_FWD_Z  (z_{i-1} gate_i) Wzu_i, continuing FWD_Y's accumulator, + epilogue
//   FC_UNIT_DELTA  delta_i Wzu_i^T (-> delta_{i-1})   FC_UNIT_DEDY  delta_i Wyu_i^T (-> gbuf)   FC_UNIT_E  one energy row
// Tile t of a GEMM belongs to wave t % NWAVE in the interval of its layer (fc_home_wave), and the narrow GEMMs leave waves idle
// there.  fc_deal moves the DEDY units, which need less than their interval's barrier provides: DEDY of layer i+1 reads
// delta_{i+1}, which interval i+1 already had, and runs in the backward interval of layer i on the waves with the shortest
// chains there (counted in k-blocks, ties to the highest wave) -- if dE/dy has at most one tile per wave.  DEDY of layer 0
// stays, keeps its accumulator across the last barrier and forms g = gscale * fma(cyu_0, acc, gbuf) from there, so gbuf sees
// the same fma chain L-1 .. 0 per element and the separate pass that stored g is gone.  With more than NWAVE tiles of dE/dy
// every unit stays at home (same bits).  The energy rows ride in the last interval, row by row onto the shortest chains.
// (Measured and left out, DESIGN.md section 6: FWD_Y of a narrow layer an interval early with the accumulator carried across the
//  barrier, and the energy rows in the first backward interval.)
enum { FC_UNIT_FWD_Y = 0, FC_UNIT_FWD_Z = 1, FC_UNIT_DELTA = 2, FC_UNIT_DEDY = 3, FC_UNIT_E = 4 };
constexpr int FC_E_ROW_COST = 2;      // an energy row, in k-blocks of a GEMM chain (one memory round trip and a few fmas)
// the wave with the shortest chain (ties: the highest)
constexpr int fc_deal_pick(const int *load) {
    int best = NWAVE - 1;
    for (int w = NWAVE - 2; w >= 0; --w)
        if (load[w] < load[best]) best = w;
    return best;
}
constexpr FcDeal fc_deal(int n, int L, const int *width) {
    FcDeal d{};
    const int NTy = pad16(n) / 16;
    d.bwd_moved = NTy <= NWAVE;
    for (int i = L - 1; i >= 0; --i) {                   // backward interval of layer i
        int load[NWAVE] = {};
        if (i > 0)
            for (int t = 0; t < pad16(width[i - 1]) / 16; ++t) load[t % NWAVE] += kblocks_tile(width[i]);
        if (d.bwd_moved) {
            if (i == 0)
                for (int t = 0; t < NTy; ++t) {
                    d.dy_mask[0][t] = (unsigned short)(1u << t);
                    load[t] += kblocks_tile(width[0]);
                }
            if (i + 1 < L)
                for (int t = 0; t < NTy; ++t) {
                    const int w = fc_deal_pick(load);
                    d.dy_mask[i + 1][w] |= (unsigned short)(1u << t);
                    load[w] += kblocks_tile(width[i + 1]);
                }
        } else {
            for (int t = 0; t < NTy; ++t) load[i > 0 ? NWAVE - 1 - t % NWAVE : t % NWAVE] += kblocks_tile(width[i]);
        }
        if (i == 0)
            for (int r = 0; r < TM; ++r) {
                const int w = fc_deal_pick(load);
                d.e_mask[w] |= (unsigned short)(1u << r);
                load[w] += FC_E_ROW_COST;
            }
    }
    return d;
}
// the wave of tile t of a GEMM the deal leaves in the interval of its layer (DEDY: with a DELTA product behind it in the same
// interval, i > 0, the few dE/dy tiles are counted from the top -- those waves have the fewest delta tiles)
__host__ __device__ constexpr int fc_home_wave(int t) { return t % NWAVE; }
__host__ __device__ constexpr int fc_home_wave_dedy(int layer, int t) { return layer > 0 ? NWAVE - 1 - t % NWAVE : t % NWAVE; }

// 0, or ICNN_BE_EINVAL: not a network (no hidden layer, too many, a width below 1, a final width other than 1)
// R: the rows of the evaluation tile (TM, 8 or 4) -- the LDS buffers hold R rows each, nothing else depends on it
constexpr int fc_geom(int n, int n_layers, const int *width, FcGeom &a, int R = TM) {
    const int L = n_layers - 1;
    if (L < 1 || n_layers > ICNN_BE_MAX_LAYERS || width[L] != 1 || n < 1) return ICNN_BE_EINVAL;
    if (R != TM && R != 8 && R != 4) return ICNN_BE_EINVAL;
    a.lds_rows = R;
    a.n = n;
    a.L = L;
    int o = 0, lo = 0;
    for (int i = 0; i <= L; ++i) {
        if (width[i] < 1) return ICNN_BE_EINVAL;
        a.width[i] = width[i];
        a.yu_off[i] = o; o += n;
        a.zu_off[i] = o; o += width[i];
        a.gate_off[i] = -1;
        if (i > 0) { a.gate_off[i] = o; o += width[i - 1]; }
    }
    a.ctx_width = o;
    const PackOffsets po = pack_offsets(n, n_layers, width);
    for (int i = 0; i <= L; ++i) {
        a.w_yu_f[i] = po.yu_f[i]; a.w_yu_b[i] = po.yu_b[i];
        a.w_zu_f[i] = po.zu_f[i]; a.w_zu_b[i] = po.zu_b[i];
    }
    a.ldY = lds_pitch(n);
    a.ybuf_off = lo; lo += R * a.ldY;
    for (int i = 0; i < L; ++i) { a.aop_off[i] = lo; lo += R * a.ldY; }
    a.gbuf_off = lo; lo += R * a.ldY;
    for (int i = 0; i < L; ++i) {
        a.zb_ld[i] = lds_pitch(width[i]);
        a.zb_off[i] = lo; lo += R * a.zb_ld[i];
    }
    a.dl_off = lo; lo += R * a.zb_ld[L - 1];
    a.lds_floats = lo;
    a.deal = fc_deal(n, L, width);
    return 0;
}
// dst (FcArgs or FcGeom) <- the geometry; same(): every geometry field of `a` is g's
template <typename Dst>
constexpr void fc_geom_copy(Dst &d, const FcGeom &g) {
    d.n = g.n; d.L = g.L; d.ctx_width = g.ctx_width;
    d.ldY = g.ldY; d.ybuf_off = g.ybuf_off; d.gbuf_off = g.gbuf_off; d.dl_off = g.dl_off; d.lds_floats = g.lds_floats;
    d.lds_rows = g.lds_rows;
    d.deal = g.deal;
    for (int i = 0; i < ICNN_BE_MAX_LAYERS; ++i) {
        d.width[i] = g.width[i];
        d.yu_off[i] = g.yu_off[i]; d.zu_off[i] = g.zu_off[i]; d.gate_off[i] = g.gate_off[i];
        d.w_yu_f[i] = g.w_yu_f[i]; d.w_yu_b[i] = g.w_yu_b[i]; d.w_zu_f[i] = g.w_zu_f[i]; d.w_zu_b[i] = g.w_zu_b[i];
        d.zb_off[i] = g.zb_off[i]; d.zb_ld[i] = g.zb_ld[i]; d.aop_off[i] = g.aop_off[i];
    }
}
template <typename A>
constexpr bool fc_geom_same(const A &a, const FcGeom &g) {
    bool ok = a.n == g.n && a.L == g.L && a.ctx_width == g.ctx_width && a.ldY == g.ldY && a.ybuf_off == g.ybuf_off &&
              a.gbuf_off == g.gbuf_off && a.dl_off == g.dl_off && a.lds_floats == g.lds_floats && a.lds_rows == g.lds_rows;
    for (int i = 0; i < ICNN_BE_MAX_LAYERS; ++i)
        ok = ok && a.width[i] == g.width[i] && a.yu_off[i] == g.yu_off[i] && a.zu_off[i] == g.zu_off[i] &&
             a.gate_off[i] == g.gate_off[i] && a.w_yu_f[i] == g.w_yu_f[i] && a.w_yu_b[i] == g.w_yu_b[i] &&
             a.w_zu_f[i] == g.w_zu_f[i] && a.w_zu_b[i] == g.w_zu_b[i] && a.zb_off[i] == g.zb_off[i] &&
             a.zb_ld[i] == g.zb_ld[i] && a.aop_off[i] == g.aop_off[i];
    return ok;
}

// The fixed shape policy (be_kernels.h): y of N entries, layer widths W... (the last one is the scalar head's 1).
template <int N, int... W>
struct FixedShape : FixedDual<N> {
    static constexpr int N_LAYERS = (int)sizeof...(W);
    static constexpr int LAYER_UNROLL = ICNN_BE_MAX_LAYERS;     // the layer loops of fc_fg_tile unroll completely
    static constexpr FcGeom make() {
        const int w[ICNN_BE_MAX_LAYERS] = {W...};
        FcGeom g{};
        fc_geom(N, N_LAYERS, w, g);
        return g;
    }
    static constexpr FcGeom GEOM = make();
    static_assert(N_LAYERS >= 2 && N_LAYERS <= ICNN_BE_MAX_LAYERS && GEOM.L == N_LAYERS - 1, "not a network");
    static_assert(GEOM.lds_floats * 4 <= LDS_BYTES, "the tile's activation buffers do not fit the LDS");
    static_assert(GEOM.lds_rows == TM, "the fixed instances are 16-row tiles");
    template <typename A> static __device__ __forceinline__ const FcGeom &fc(const A &) { return GEOM; }
};

__device__ __forceinline__ float act_fn(float p, float alpha) { return p > 0.f ? p : alpha * p; }

// acc{0,1} += A[16][K] (LDS, pitch ld) * packed weight tiles nt0 / nt1 (nt1 < 0: only one tile; with TILE_PAIR off that is
// every call).  Two output tiles would share every A fragment read.  The B fragments (16 B per lane from L2) run an RD-deep
// register ring ahead of the MFMAs and the A fragment of the next k-block is read before the MFMAs of the current one.  KB is a
// multiple of RD (kblocks_tile: the real k-blocks; the LDS pad columns behind them are zero), the one- and two-tile cases are
// separate loops and the tile indices are wave-uniform: the loop body is straight-line code whose accumulators and ring slots
// never change registers (a copy of an MFMA result drains the matrix pipe; a copy of a fragment waits for its load).  What the
// machine code has to look like, and what it took (round 4, read off the ISA): the first RD requests in the order of use --
// otherwise the wait-count pass, merging that order with the loop's at the loop header, drains the ring with vmcnt(0) in every
// turn --, and a slot's refill behind the MFMAs that read it.
// Per output element the accumulation is the k-ordered fma chain oracle/picnn_chain.c reproduces.
// A narrow tile (A holds R = 8 or 4 rows, gemm_tiles' rmask = R - 1): an MFMA output row depends on its own A row alone, so the
// lanes of rows >= R gather row r16 & rmask -- a valid one -- and the callers drop their outputs.  One AND in front of the loop.
//
// `pre` (the first GEMM of a unit): the requests of the unit's epilogue operands -- eight or nine context loads per lane that
// miss the L2 --, issued BEHIND the ring's first RD requests.  The vector-memory counter retires in order: requested in front
// of the ring, every one of them had to land before the first MFMA of the unit could start.  The first turn of the loop is then
// taken outside it: a wait at the loop header is one instruction for every turn and has to assume the back edge's state (only
// the refills outstanding), so inside the loop the first turn would wait for `pre`'s loads all the same; peeled, its waits
// count them as younger than the fragments and leave them in flight, and the first refill's wait at the loop header is the
// first that covers them.
struct NoPre {
    __device__ __forceinline__ void operator()() const {}
};
template <bool TWO, int RD, typename Pre>   // RD: depth of the fragment ring = unroll factor; KB a multiple of it
__device__ __forceinline__ void gemm_loop(const float *ap, const f4 *bp0, const f4 *bp1, size_t kstride, int KB,
                                          f4 &acc0, f4 &acc1, Pre pre) {
    constexpr bool PEEL = !__is_same(Pre, NoPre);
    f4 b0[RD], b1[RD];
#pragma unroll
    for (int d = 0; d < RD; ++d) {       // issued in the order of use, pinned: the wait-count pass merges this order with the
        b0[d] = bp0[(size_t)d * kstride];   // loop's own at the loop header, and a fragment requested out of turn here costs
        __builtin_amdgcn_sched_barrier(0);  // a full drain of the ring (s_waitcnt vmcnt(0)) in EVERY turn of the loop
        if (TWO) {
            b1[d] = bp1[(size_t)d * kstride];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    pre();
    __builtin_amdgcn_sched_barrier(0);
    f4 an = *reinterpret_cast<const f4 *>(ap);
    auto turn = [&](int kb0) {
#pragma unroll
        for (int d = 0; d < RD; ++d) {
            const int kb = kb0 + d;
            const f4 a = an;
            an = *reinterpret_cast<const f4 *>(ap + (kb + 1 < KB ? kb + 1 : kb) * 16);
            const f4 x0 = b0[d], x1 = b1[d];
            const int nk = kb + RD < KB ? kb + RD : kb;          // ring refill (clamped re-read at the tail)
            if (TWO) {
                b0[d] = bp0[(size_t)nk * kstride];
                b1[d] = bp1[(size_t)nk * kstride];
            }
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, x0.x, acc0, 0, 0, 0);
            if (TWO) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, x1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, x0.y, acc0, 0, 0, 0);
            if (TWO) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, x1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, x0.z, acc0, 0, 0, 0);
            if (TWO) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, x1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, x0.w, acc0, 0, 0, 0);
            if (TWO) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, x1.w, acc1, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < (TWO ? 8 : 0); ++g) {            // one MFMA, then up to two other instructions
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x126, 2, 0);
            }
            if (!TWO) {
                // one tile per wave: the slot is refilled BEHIND the MFMAs that read it, pinned there -- requested in front
                // of them the new fragment needs a second register and a copy, and the copy waits for the load on the spot
                __builtin_amdgcn_sched_barrier(0);
                b0[d] = bp0[(size_t)nk * kstride];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    if (PEEL && KB > 0) turn(0);
    for (int kb0 = PEEL ? RD : 0; kb0 < KB; kb0 += RD) turn(kb0);
}
template <typename Pre = NoPre>
__device__ __forceinline__ void gemm_tiles(const float *A, int ld, int rmask, const float *Wp, int KB, int NT, int nt0, int nt1,
                                           f4 &acc0, f4 &acc1, Pre pre = Pre{}) {
    const int lane = thread_id() & 63, r16 = lane & 15, q = lane >> 4;
    nt0 = __builtin_amdgcn_readfirstlane(nt0);
    nt1 = __builtin_amdgcn_readfirstlane(nt1);
    const float *ap = A + (r16 & rmask) * ld + 4 * q;
    const f4 *bp0 = reinterpret_cast<const f4 *>(Wp) + (size_t)nt0 * 64 + lane;
    const f4 *bp1 = reinterpret_cast<const f4 *>(Wp) + (size_t)(nt1 >= 0 ? nt1 : nt0) * 64 + lane;
    const size_t kstride = (size_t)NT * 64;              // f4 elements between consecutive k-blocks of a tile
    static_assert(TILE_RD == 2, "the odd k-block below");
    const int KBe = KB & ~1;
    if (TILE_PAIR && nt1 >= 0) gemm_loop<true, TILE_RD>(ap, bp0, bp1, kstride, KBe, acc0, acc1, pre);
    else gemm_loop<false, TILE_RD>(ap, bp0, bp1, kstride, KBe, acc0, acc1, pre);
    // (see kblocks_tile: rare widths; one k-block without a ring behind the loop.  A second loop instance with a ring of PF for
    //  them -- never executed on the benchmark's network -- cost it 3 %: 1.069 against 1.038 ms on one box)
    if (KB & 1) {
        const f4 a = *reinterpret_cast<const f4 *>(ap + KBe * 16);
        const f4 x0 = bp0[(size_t)KBe * kstride];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, x0.x, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, x0.y, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, x0.z, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, x0.w, acc0, 0, 0, 0);
        if (nt1 >= 0) {
            const f4 x1 = bp1[(size_t)KBe * kstride];
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, x1.x, acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, x1.y, acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, x1.z, acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, x1.w, acc1, 0, 0, 0);
        }
    }
}

// (A of TM rows: be_ficnn.hip)
template <typename Pre = NoPre>
__device__ __forceinline__ void gemm_tiles(const float *A, int ld, const float *Wp, int KB, int NT, int nt0, int nt1,
                                           f4 &acc0, f4 &acc1, Pre pre = Pre{}) {
    gemm_tiles(A, ld, TM - 1, Wp, KB, NT, nt0, nt1, acc0, acc1, pre);
}

// One tile of TM samples (workgroup-wide: NTHREADS threads, `lds` = the dynamic shared memory of the workgroup).
// Stand-alone kernel: one workgroup per tile.  be_fused.hip calls it once per round from its persistent workgroup.
// Shape (be_kernels.h): where the geometry comes from -- the arguments (DynShape), or constants (FixedShape: `ge` below is a
// constant object, the layer loops unroll, and every gemm_tiles call sees constant KB, NT, strides and LDS pitches)
template <typename Shape = DynShape, typename ArgsT>   // ArgsT: FcArgs by value, or a reference into the kernel-argument segment (be_fused.hip)
__device__ __forceinline__ void fc_fg_tile(const ArgsT &a, int tile, float *lds) {
    // Every float32 operation below is written out (explicit fmaf, no compiler contraction) so that
    // oracle/picnn_chain.c can reproduce the kernel's result bit for bit.
#pragma clang fp contract(off)
    const int tid = thread_id(), lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const auto &ge = Shape::fc(a);
    const int TR = a.tile_rows;
    const int s0 = tile * TR;
    const int rows = min(TR, a.batch - s0);
    const int LR = ge.lds_rows, rmask = LR - 1;      // rows of the LDS buffers (a constant TM for a fixed shape); rows <= LR
    const int n = ge.n, L = ge.L, C = ge.ctx_width, ldY = ge.ldY;
    const int npad = pad16(n);
    float *ybuf = lds + ge.ybuf_off;      // y (network input)
    long long tick = ICNN_BE_PROF_ON(a.prof) ? (long long)__builtin_readcyclecounter() : 0;
    auto lap = [&](int phase) {          // diagnostic only (tools/fc_phase_profile.py; it knows the slots of up to two layers)
        if (ICNN_BE_PROF_ON(a.prof) && phase < FC_PROF_PHASES) {
            const long long now = (long long)__builtin_readcyclecounter();
            if (lane == 0)
                atomicAdd(reinterpret_cast<unsigned long long *>(a.prof) +
                              ((size_t)tile * NWAVE + wave) * FC_PROF_PHASES + phase,
                          (unsigned long long)(now - tick));
            tick = now;
        }
    };

    // nothing to do if every sample of the tile has left the loop -- the flags are REQUESTED here and looked at behind the
    // first batch of input loads below (one memory round trip per evaluation instead of two in a row)
    int live = 1;
    if (a.finished) {
        live = 0;
        if (tid < rows) live = a.finished[s0 + tid] == 0;
    }
    const float *ctx = a.ctx + (size_t)s0 * C;
    float *gbuf = lds + ge.gbuf_off;      // dE/dy accumulator of the backward pass
    float *dl = lds + ge.dl_off;          // delta_{L-1} (the activations z_{L-1} stay intact for the energy)

    // Wave w prepares row w of the tile (TM == NWAVE): no index arithmetic beyond lane strides.  A narrow tile has rows for
    // the first LR waves only: the others load nothing (their row is none of the batch's) and store nothing.
    // The GEMMs read k-blocks up to a multiple of PF, i.e. pad columns [pad16(width), pitch) that no phase writes:
    // zero them (their packed weights are zero, but 0 * stale-NaN would not be).  Everything below pad16(width) is
    // written for all TM rows by the phase that produces the buffer.
    static_assert(TM == NWAVE, "one wave per row in the preparation phase");
    {
        auto zero_pad = [&](float *buf, int ld, int width) {
            const int w16 = pad16(width);
            if (wave < LR)
                for (int j = w16 + lane; j < ld; j += 64) buf[wave * ld + j] = 0.f;
        };
        for (int i = 0; i < L; ++i) zero_pad(lds + ge.aop_off[i], ldY, n);
        for (int i = 0; i < L; ++i) zero_pad(lds + ge.zb_off[i], ge.zb_ld[i], ge.width[i]);
        zero_pad(dl, ge.zb_ld[L - 1], ge.width[L - 1]);
    }
    // network input: y rounded to float32 like a TensorFlow feed (RL wrapper feeds 2y-1), and with it the y-operand
    // y * yu_i of EVERY layer; all loads of a lane's elements are issued before the first use
    {
        const int r = wave;
        const bool row_ok = r < rows;
        for (int j0 = 0; j0 < npad; j0 += 4 * 64) {
            double yd[4];
            float cu[4][ICNN_BE_MAX_LAYERS];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j0 + 64 * k + lane;
                const bool ok = row_ok && j < n;
                yd[k] = ok ? a.y[(size_t)(s0 + r) * n + j] : 0.0;
#pragma unroll
                for (int i = 0; i < ICNN_BE_MAX_LAYERS; ++i)
                    cu[k][i] = ok && i < L ? ctx[(size_t)r * C + ge.yu_off[i] + j] : 0.f;
            }
            if (j0 == 0 && a.finished && !__syncthreads_or(live)) return;     // (uniform: every thread takes j0 = 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j0 + 64 * k + lane;
                if (j < npad && r < LR) {
                    const float v = a.action_box ? (float)(2.0 * yd[k] - 1.0) : (float)yd[k];
                    const bool ok = row_ok && j < n;
                    ybuf[r * ldY + j] = ok ? v : 0.f;
#pragma unroll
                    for (int i = 0; i < ICNN_BE_MAX_LAYERS; ++i)
                        if (i < L) lds[ge.aop_off[i] + r * ldY + j] = ok ? v * cu[k][i] : 0.f;
                }
            }
        }
    }
    __syncthreads();
    lap(0);

    // ---------------- forward ------------------------------------------------------------
    static_assert(!TILE_PAIR, "the dE/dy_0 unit carries ONE accumulator across the last barrier");
    const auto &deal = ge.deal;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const float *wyL = a.wpack + ge.w_yu_f[L];       // final scalar layer: plain vectors
    const float *wzL = a.wpack + ge.w_zu_f[L];
    const int KBy = kblocks_tile(n);
#pragma unroll(Shape::LAYER_UNROLL)
    for (int i = 0; i < L; ++i) {
        const int wi = ge.width[i], wpad = pad16(wi);
        const bool last = i == L - 1;
        float *zout = lds + ge.zb_off[i];
        const int ldo = ge.zb_ld[i];
        const int NT = wpad / 16;
        const float *Wy = a.wpack + ge.w_yu_f[i];
        for (int nt = fc_home_wave(wave); nt < NT; nt += TILE_STEP) {
            const int nt1 = -1;
            f4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            // epilogue operands (x-only context): requested in front of the MFMA loops so that their HBM/L2 latency is hidden
            // behind them, but behind the first weight fragments of the unit (gemm_loop, `pre`).  Every lane loads, rows and
            // columns outside the tile from row 0 / column 0 of it: a load under a branch cannot be counted by the wait in
            // front of the first MFMA, which then assumes none was issued and waits for all of them.  The epilogues read the
            // operands of real rows and columns only.
            float czu[2][4], cgt[2][4], wz[2];
            auto operands = [&] {
#pragma unroll
                for (int h = 0; h < (TILE_PAIR ? 2 : 1); ++h) {
                    const int tile = h == 0 ? nt : nt1;
                    const int col = tile * 16 + r16;
                    const int cc = tile >= 0 && col < wi ? col : 0;
                    wz[h] = wzL[last ? cc : 0];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 4 * q + r;
                        const float *c = ctx + (size_t)(row < rows ? row : 0) * C;
                        czu[h][r] = c[ge.zu_off[i] + cc];
                        cgt[h][r] = c[ge.gate_off[i + 1] + cc];
                    }
                }
            };
            gemm_tiles(lds + ge.aop_off[i], ldY, rmask, Wy, KBy, NT, nt, nt1, acc[0], acc[1], operands);
            if (i > 0)
                gemm_tiles(lds + ge.zb_off[i - 1], ge.zb_ld[i - 1], rmask, a.wpack + ge.w_zu_f[i],
                           kblocks_tile(ge.width[i - 1]), NT, nt, nt1, acc[0], acc[1]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int tile = h == 0 ? nt : nt1;
                if (tile < 0) continue;
                const int col = tile * 16 + r16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * q + r;
                    float v = 0.f, d = 0.f;
                    if (row < rows && col < wi) {
                        const float z = act_fn(acc[h][r] + czu[h][r], a.alpha);
                        v = z * cgt[h][r];                    // operand of the next layer: z_i * gate_{i+1}
                        // last hidden layer: delta_{L-1} = gate_L * wzu_L * act'(pre); sign(pre) = sign(z * gate), gate > 0
                        const float gw = cgt[h][r] * wz[h];
                        d = gw * (v > 0.f ? 1.f : a.alpha);
                    }
                    if (row < LR) {                           // (a narrow tile has no such row: its output is dropped)
                        zout[row * ldo + col] = v;
                        if (last) dl[row * ldo + col] = d;
                    }
                }
            }
        }
        lap(2 + 3 * i);
        __syncthreads();
        lap(3 + 3 * i);
    }

    // ---------------- backward (the energy of the final scalar layer rides along in its last interval) ---------
    const int NTy = npad / 16;
    const bool bmoved = deal.bwd_moved;
    f4 gacc = {0.f, 0.f, 0.f, 0.f};                  // dE/dy_0 of this wave's tile and its operand, kept across the last barrier
    float gcyu[4] = {0.f, 0.f, 0.f, 0.f};
    int gtile = -1;
    // one tile of dE/dy (+)= yu_j * (delta_j Wyu_j^T), starting from yu_L * wyu_L; `defer`: the fma into gbuf is left to the caller
    auto dy_unit = [&](int j, int nt, bool defer) {
        const bool first = j == L - 1;
        const float *delta = first ? dl : lds + ge.zb_off[j];
        f4 acc = {0.f, 0.f, 0.f, 0.f}, none = {0.f, 0.f, 0.f, 0.f};
        float cyu[4], cyL[4], wy;
        // (not the first backward layer: cyL is not used; its loads repeat cyu's addresses)
        const int offL = first ? ge.yu_off[L] : ge.yu_off[j];
        const int col = nt * 16 + r16;
        auto operands = [&] {
            const int cc = col < n ? col : 0;
            wy = wyL[first ? cc : 0];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                const float *c = ctx + (size_t)(row < rows ? row : 0) * C;
                cyu[r] = c[ge.yu_off[j] + cc];
                cyL[r] = c[offL + cc];
            }
        };
        gemm_tiles(delta, ge.zb_ld[j], rmask, a.wpack + ge.w_yu_b[j], kblocks_tile(ge.width[j]), NTy, nt, -1, acc, none, operands);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * q + r;
            if (row < rows && col < n) {
                const float g_in = first ? cyL[r] * wy : gbuf[row * ldY + col];
                if (!defer) gbuf[row * ldY + col] = __builtin_fmaf(cyu[r], acc[r], g_in);
                else if (first) gbuf[row * ldY + col] = g_in;
            }
            gcyu[r] = defer ? cyu[r] : gcyu[r];
        }
        if (defer) {
            gacc = acc;
            gtile = nt;
        }
    };
#pragma unroll(Shape::LAYER_UNROLL)
    for (int i = L - 1; i >= 0; --i) {
        const int wi = ge.width[i];
        const bool first = i == L - 1;
        const float *delta = first ? dl : lds + ge.zb_off[i];
        const int ldd = ge.zb_ld[i], KB = kblocks_tile(wi);
        if (!bmoved)
            for (int nt = fc_home_wave_dedy(i, wave); nt < NTy; nt += TILE_STEP) dy_unit(i, nt, false);
        if (i > 0) {   // delta_{i-1} = gate_i * (delta_i Wzu_i^T) * act'(pre_{i-1})
            const int wp = ge.width[i - 1];
            float *zprev = lds + ge.zb_off[i - 1];
            const int ldp = ge.zb_ld[i - 1];
            const float *Wt = a.wpack + ge.w_zu_b[i];
            const int NTp = pad16(wp) / 16;
            for (int nt = fc_home_wave(wave); nt < NTp; nt += TILE_STEP) {
                f4 acc = {0.f, 0.f, 0.f, 0.f}, none = {0.f, 0.f, 0.f, 0.f};
                float cga[4];
                const int col = nt * 16 + r16;
                auto operands = [&] {
                    const int cc = col < wp ? col : 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 4 * q + r;
                        cga[r] = ctx[(size_t)(row < rows ? row : 0) * C + ge.gate_off[i] + cc];
                    }
                };
                gemm_tiles(delta, ldd, rmask, Wt, KB, NTp, nt, -1, acc, none, operands);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * q + r;
                    float d = 0.f;
                    if (row < rows && col < wp) {
                        const float gate = cga[r];
                        const float ga = gate * acc[r];
                        d = ga * (zprev[row * ldp + col] > 0.f ? 1.f : a.alpha);
                    }
                    if (row < LR) zprev[row * ldp + col] = d;
                }
            }
        }
        if (bmoved && i == 0 && deal.dy_mask[0][wv]) dy_unit(0, __builtin_ctz(deal.dy_mask[0][wv]), true);
        lap(i == 0 ? 10 : 8);
        if (bmoved && i + 1 < L)     // dE/dy of the layer behind: its delta is a whole interval old
            for (unsigned m = deal.dy_mask[i + 1][wv]; m; m &= m - 1) dy_unit(i + 1, __builtin_ctz(m), false);
        if (i == 0) lap(11);
        if (i == 0) {
            // E = z_{L-1} . wzu_L + (y * yu_L) . wyu_L + zu_L, a row per wave at a time (two, where the deal gives a wave more
            // than one): every operand of the pair's first 256 columns is requested before the first fma
            const float *zl = lds + ge.zb_off[L - 1];
            const int ldz = ge.zb_ld[L - 1], wl = ge.width[L - 1];
            unsigned m = rows > 0 ? deal.e_mask[wv] & ((1u << rows) - 1u) : 0u;
            while (m) {
                int rr[2];
                rr[0] = rr[1] = __builtin_ctz(m);
                m &= m - 1;
                const bool two = m != 0;
                if (two) {
                    rr[1] = __builtin_ctz(m);
                    m &= m - 1;
                }
                const float *c[2] = {ctx + (size_t)rr[0] * C, ctx + (size_t)rr[1] * C};
                float part[2] = {0.f, 0.f}, cy[2][4], wyv[4], czL[2];
                auto y_loads = [&](int j0) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = j0 + 64 * k + lane, jc = j < n ? j : 0;
                        wyv[k] = wyL[jc];
#pragma unroll
                        for (int h = 0; h < 2; ++h) cy[h][k] = c[h][ge.yu_off[L] + jc];
                    }
                };
                y_loads(0);
#pragma unroll
                for (int h = 0; h < 2; ++h) czL[h] = c[h][ge.zu_off[L]];
                for (int j0 = 0; j0 < wl; j0 += 256) {
                    float wzv[4], zv[2][4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = j0 + 64 * k + lane, jc = j < wl ? j : 0;
                        wzv[k] = wzL[jc];
#pragma unroll
                        for (int h = 0; h < 2; ++h) zv[h][k] = zl[rr[h] * ldz + jc];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int h = 0; h < 2; ++h)
                            part[h] = j0 + 64 * k + lane < wl ? __builtin_fmaf(zv[h][k], wzv[k], part[h]) : part[h];
                }
                for (int j0 = 0; j0 < n; j0 += 256) {
                    if (j0 > 0) y_loads(j0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = j0 + 64 * k + lane, jc = j < n ? j : 0;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const float yy = ybuf[rr[h] * ldY + jc] * cy[h][k];
                            part[h] = j < n ? __builtin_fmaf(yy, wyv[k], part[h]) : part[h];
                        }
                    }
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float e = wave_sum_f(part[h]) + czL[h];
                    if (lane == 0 && (h == 0 || two)) a.f[s0 + rr[h]] = e;
                }
            }
            lap(7);
        }
        __syncthreads();
        lap(i == 0 ? 12 : 9);
    }

    const float gscale = a.action_box ? 2.f : 1.f;    // RL/src/icnn.py:152  grad *= 2
    if (!bmoved) {
        if (wave < rows)
            for (int j = lane; j < n; j += 64) a.g[(size_t)(s0 + wave) * n + j] = gscale * gbuf[wave * ldY + j];
    } else if (gtile >= 0) {   // g = gscale * (dE/dy_0's fma into gbuf): the chain of this wave's tile ends here, behind the barrier
        const int col = gtile * 16 + r16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * q + r;
            if (row < rows && col < n)
                a.g[(size_t)(s0 + row) * n + col] = gscale * __builtin_fmaf(gcyu[r], gacc[r], gbuf[row * ldY + col]);
        }
    }
    lap(13);
}


// rows of the model's evaluation tile: TM (tile_rows 0 or 16), a narrow tile (8, 4), or 0: not a tile
inline int fc_model_rows(const icnn_be_fc_model &m) {
    return m.tile_rows == 0 || m.tile_rows == TM ? TM : m.tile_rows == 8 || m.tile_rows == 4 ? m.tile_rows : 0;
}
inline bool fc_model_narrow(const icnn_be_fc_model &m) { return fc_model_rows(m) != TM; }

inline int fill_args(const icnn_be_fc_model &m, FcArgs &a, int &lds_bytes) {
    FcGeom g{};
    const int R = fc_model_rows(m);
    if (R == 0) return ICNN_BE_EINVAL;
    if (int rc = fc_geom(m.n, m.n_layers, m.width, g, R)) return rc;
    if (g.ctx_width != m.ctx_width) return ICNN_BE_EINVAL;
    fc_geom_copy(a, g);
    a.alpha = m.alpha;
    a.action_box = m.action_box;
    a.tile_rows = R;
    lds_bytes = g.lds_floats * 4;
    if (lds_bytes > LDS_BYTES) return ICNN_BE_ELIMIT;
    a.wpack = m.wpack;
    return 0;
}

}  // namespace
}  // namespace icnn_be
