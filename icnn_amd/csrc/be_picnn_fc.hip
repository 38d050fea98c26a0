// FC-PICNN energy/gradient: kernel wrapper, weight packing entry points, launcher (device code: be_picnn_fc_dev.h).
#include "be_picnn_fc_dev.h"
#include "be_picnn_fc_rows_dev.h"

namespace icnn_be {

namespace {

__global__ __launch_bounds__(NTHREADS) void fc_fg_kernel(FcArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fc_fg_tile(a, blockIdx.x, lds);
}

// Batches of at most one sample per CU: a workgroup per sample on the VALU path (be_picnn_fc_rows_dev.h) instead of
// 16-row MFMA tiles that would be mostly empty rows on a few CUs.  Same results bit for bit.
struct FgRowsArgs {
    FcArgs fa;
    RowsLayout lay;
    int per_wg;
};
__global__ __launch_bounds__(RTHREADS) void fc_fg_rows_kernel(FgRowsArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const FcArgs &fa = a.fa;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = fa.n, RF = a.lay.row_floats;
    const int s_base = blockIdx.x * a.per_wg;
    const int batch = fa.batch - s_base < a.per_wg ? fa.batch - s_base : a.per_wg;
    if (fa.finished) {                   // nothing to do if every sample of the workgroup has left the loop
        int live = 0;
        if (tid < batch) live = fa.finished[s_base + tid] == 0;
        if (!__syncthreads_or(live)) return;
    }
    rows_setup(fa, a.lay, lds, s_base, batch, tid);
    if (wave < batch) {                  // network input: y rounded to float32 like a TensorFlow feed; RL wrapper feeds 2y-1
        float *row = lds + wave * RF;
        for (int j = lane; j < n; j += 64) {
            const double yd = fa.y[(size_t)(s_base + wave) * n + j];
            rows_set_input(fa, a.lay, row, j, fa.action_box ? (float)(2.0 * yd - 1.0) : (float)yd);
        }
    }
    __syncthreads();
    rows_eval(fa, a.lay, lds, batch, tid, [](int) {});
    if (wave < batch) {
        const float *row = lds + wave * RF;
        const float gscale = fa.action_box ? 2.f : 1.f;    // RL/src/icnn.py:152  grad *= 2
        if (lane == 0) fa.f[s_base + wave] = lds[a.lay.f_off + wave];
        for (int j = lane; j < n; j += 64) fa.g[(size_t)(s_base + wave) * n + j] = gscale * row[a.lay.g_off + j];
    }
}

}  // namespace

static long long *g_fc_prof = nullptr;
void set_fc_profile_buffer(long long *buf) { g_fc_prof = buf; }
long long *fc_profile_buffer() { return g_fc_prof; }

size_t fc_pack_floats(const icnn_be_fc_model &m) { return pack_offsets(m).total; }

int fc_pack(const icnn_be_fc_model &m, const float *const *w_yu, const float *const *w_zu, float *out) {
    const PackOffsets o = pack_offsets(m);
    const int L = m.n_layers - 1;
    for (size_t i = 0; i < o.total; ++i) out[i] = 0.f;
    for (int i = 0; i <= L; ++i) {
        const int wi = m.width[i];
        if (i < L) {
            pack_operand(w_yu[i], m.n, wi, false, out + o.yu_f[i]);      // forward:  [n] x [wi]
            pack_operand(w_yu[i], wi, m.n, true, out + o.yu_b[i]);       // backward: Wyu^T
            if (i > 0) {
                pack_operand(w_zu[i], m.width[i - 1], wi, false, out + o.zu_f[i]);
                pack_operand(w_zu[i], wi, m.width[i - 1], true, out + o.zu_b[i]);
            }
        } else {
            for (int j = 0; j < m.n; ++j) out[o.yu_f[i] + j] = w_yu[i][j];
            for (int j = 0; j < m.width[i - 1]; ++j) out[o.zu_f[i] + j] = w_zu[i][j];
        }
    }
    return 0;
}

hipError_t launch_fc_fg(const icnn_be_fc_model &m, const float *ctx, const double *y, int batch,
                        float *f, float *g, const int *finished, hipStream_t stream) {
    FcArgs a{};
    int lds = 0;
    if (fill_args(m, a, lds) != 0) return hipErrorInvalidValue;
    a.ctx = ctx; a.y = y; a.f = f; a.g = g; a.finished = finished; a.batch = batch;
    a.prof = g_fc_prof;
    if (!g_fc_prof) {       // (the phase profiler instruments the tile kernel)
        FgRowsArgs r{};
        int rows_lds = 0;
        if (const int per_wg = rows_per_wg(m, batch, 0, r.lay, rows_lds)) {        // at most two samples per CU
            r.fa = a;
            r.per_wg = per_wg;
            return launch_kernel(fc_fg_rows_kernel, dim3((batch + per_wg - 1) / per_wg), dim3(RTHREADS), rows_lds, stream, r);
        }
    }
    return launch_kernel(fc_fg_kernel, dim3((batch + a.tile_rows - 1) / a.tile_rows), dim3(NTHREADS), lds, stream, a);
}

hipError_t launch_fc_clamp(const icnn_be_fc_model &m, int mode, hipStream_t stream) {
    const PackOffsets o = pack_offsets(m);
    const int L = m.n_layers - 1;
    float *w = const_cast<float *>(m.wpack);
    for (int i = 1; i <= L; ++i) {
        if (i < L) {
            const size_t cnt = packed_floats(m.width[i - 1], m.width[i]);
            hipError_t e = launch_clamp(w + o.zu_f[i], cnt, mode, stream);
            if (e == hipSuccess) e = launch_clamp(w + o.zu_b[i], packed_floats(m.width[i], m.width[i - 1]), mode, stream);
            if (e != hipSuccess) return e;
        } else {
            hipError_t e = launch_clamp(w + o.zu_f[i], (size_t)pad16(m.width[i - 1]), mode, stream);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

int fc_check_model(const icnn_be_fc_model &m) {
    FcArgs a{};
    int lds = 0;
    return fill_args(m, a, lds);
}

bool fc_narrow_model(const icnn_be_fc_model &m) { return fc_model_narrow(m); }

// icnn_be_fc_tile_rows: the largest tile of 16, 8, 4 rows whose LDS buffers fit, whatever m.tile_rows says
int fc_tile_rows(const icnn_be_fc_model &m) {
    for (int R = TM; R >= 4; R /= 2) {
        FcGeom g{};
        if (int rc = fc_geom(m.n, m.n_layers, m.width, g, R)) return rc;
        if (g.ctx_width != m.ctx_width) return ICNN_BE_EINVAL;
        if (g.lds_floats * 4 <= LDS_BYTES) return R;
    }
    return ICNN_BE_ELIMIT;
}


// The deal as records { kind, layer, tile, interval, wave, interval of the result } (icnn_be_debug_fc_deal): read off the
// table and the home-wave rules fc_fg_tile itself follows.
int fc_deal_units(const icnn_be_fc_model &m, int *out, int cap) {
    FcGeom g{};
    if (int rc = fc_geom(m.n, m.n_layers, m.width, g)) return rc;
    static_assert(FC_UNIT_FWD_Y == ICNN_BE_UNIT_FWD_Y && FC_UNIT_FWD_Z == ICNN_BE_UNIT_FWD_Z && FC_UNIT_DELTA == ICNN_BE_UNIT_DELTA &&
                  FC_UNIT_DEDY == ICNN_BE_UNIT_DEDY && FC_UNIT_E == ICNN_BE_UNIT_E, "include/icnn_be.h");
    const FcDeal &d = g.deal;
    const int L = g.L, NTy = pad16(g.n) / 16;
    int count = 0;
    auto put = [&](int kind, int layer, int tile, int interval, int wave, int result) {
        if (count < cap) {
            const int rec[6] = {kind, layer, tile, interval, wave, result};
            for (int k = 0; k < 6; ++k) out[6 * count + k] = rec[k];
        }
        ++count;
    };
    auto bwd = [&](int layer) { return 2 * L - 1 - layer; };      // the backward interval of a layer
    for (int i = 0; i < L; ++i) {
        const int NT = pad16(g.width[i]) / 16;
        for (int t = 0; t < NT; ++t) {
            const int wave = fc_home_wave(t);
            put(FC_UNIT_FWD_Y, i, t, i, wave, i);
            if (i > 0) put(FC_UNIT_FWD_Z, i, t, i, wave, i);
        }
    }
    for (int i = L - 1; i >= 0; --i) {
        if (i > 0)
            for (int t = 0; t < pad16(g.width[i - 1]) / 16; ++t) put(FC_UNIT_DELTA, i, t, bwd(i), fc_home_wave(t), bwd(i));
        for (int t = 0; t < NTy; ++t) {
            if (!d.bwd_moved) {
                put(FC_UNIT_DEDY, i, t, bwd(i), fc_home_wave_dedy(i, t), bwd(i));
                continue;
            }
            for (int w = 0; w < NWAVE; ++w)
                if (d.dy_mask[i][w] >> t & 1) put(FC_UNIT_DEDY, i, t, bwd(i > 0 ? i - 1 : 0), w, i > 0 ? bwd(i - 1) : 2 * L);
        }
    }
    for (int r = 0; r < TM; ++r)
        for (int w = 0; w < NWAVE; ++w)
            if (d.e_mask[w] >> r & 1) put(FC_UNIT_E, L, r, bwd(0), w, bwd(0));
    return count;
}

}  // namespace icnn_be
