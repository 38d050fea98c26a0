// The rows form of be_gd_dev.h's iterate loop for the FC-PICNN, and the one FC launch of both rules: at most two samples per
// CU (rows_per_wg, the rule of launch_fc_fg) run the whole loop in a workgroup per one or two samples, context rows and the
// rule's state in LDS, on the VALU path of be_picnn_fc_rows_dev.h; larger batches, or rows that do not fit, take the tiles.
// Both paths evaluate E and dE/dy with the operations of icnn_be_fc_fg, so they agree bit for bit.
#pragma once
#include "be_gd_dev.h"
#include "be_picnn_fc_rows_dev.h"

namespace icnn_be {
namespace {

struct FcTile {           // phase A of gd_tile_loop
    template <typename A>
    static __device__ __forceinline__ void run(const A &fa, int tile, float *lds) { fc_fg_tile(fa, tile, lds); }
    template <typename A>
    static __device__ __forceinline__ int rows(const A &fa) { return fa.tile_rows; }
};

template <typename Rule>
struct GdRowsArgs {
    typename Rule::template Args<FcArgs> a;
    RowsLayout lay;
    int per_wg;
    int state_off;         // LDS floats: per sample the rule's state, Rule::lds_floats(npad) floats, behind the rows layout
};

// The body of a __global__ __launch_bounds__(RTHREADS) kernel whose only parameter is `r`; wave w owns sample s_base + w
template <typename Rule>
__device__ __forceinline__ void gd_rows_loop(const GdRowsArgs<Rule> &r) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const auto &a = r.a;
    const FcArgs &fa = a.fa;
    const RowsLayout &lay = r.lay;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = fa.n, npad = pad16(n), RF = lay.row_floats;
    const int s_base = blockIdx.x * r.per_wg, u = s_base + wave;
    const int batch = fa.batch - s_base < r.per_wg ? fa.batch - s_base : r.per_wg;
    float *st = lds + r.state_off + wave * Rule::lds_floats(npad);   // only touched by waves < batch
    rows_setup(fa, lay, lds, s_base, batch, tid);
    if (wave < batch) {
        float *row = lds + wave * RF;
        for (int j = lane; j < n; j += 64) {
            const typename Rule::Elem e = Rule::start(a, a.y0[(size_t)u * n + j]);
            Rule::lds_store(st, npad, j, e);
            rows_set_input(fa, lay, row, j, Rule::fed(e));
        }
    }
    __syncthreads();
    for (int k = 0; k < a.n_iter; ++k) {
        rows_eval(fa, lay, lds, batch, tid, [](int) {});     // ends with a workgroup barrier
        if (wave < batch) {
            float *row = lds + wave * RF;
            const typename Rule::Iter it = Rule::iter(a, u, k);
            [[maybe_unused]] double part = 0.0;
            for (int j = lane; j < n; j += 64) {
                typename Rule::Elem e = Rule::lds_load(st, npad, j);
                if constexpr (Rule::sums) part += Rule::step(it, e, &row[lay.g_off + j], j);
                else Rule::step(it, e, &row[lay.g_off + j], j);
                Rule::lds_store(st, npad, j, e);
                rows_set_input(fa, lay, row, j, Rule::fed(e));
            }
            if constexpr (Rule::sums) {
                const double sum = wave_sum(part);
                double *out = Rule::out(a, k, false);
                if (out && lane == 0) out[u] = (double)lds[lay.f_off + wave] + sum;
            }
        }
        __syncthreads();
    }
    if (wave < batch)
        for (int j = lane; j < n; j += 64) a.y[(size_t)u * n + j] = Rule::result(Rule::lds_load(st, npad, j));
    if (Rule::wants_final(a)) {
        rows_eval(fa, lay, lds, batch, tid, [](int) {});
        if (wave < batch) {
            if constexpr (Rule::sums) {
                double part = 0.0;
                for (int j = lane; j < n; j += 64) part += Rule::term(Rule::lds_load(st, npad, j));
                const double sum = wave_sum(part);
                if (lane == 0) Rule::out(a, a.n_iter, true)[u] = (double)lds[lay.f_off + wave] + sum;
            } else if (lane == 0) {
                fa.f[u] = lds[lay.f_off + wave];
            }
        }
    }
}

// Launches `a` (filled) on the rows kernel or the tile kernel; hipErrorNotSupported: neither fits the LDS (tile_lds bytes)
template <typename Rule, typename A>
hipError_t launch_fc_gd_rule(const icnn_be_fc_model &m, const A &a, int batch, int tile_lds, void (*tile_kernel)(A),
                             void (*rows_kernel)(GdRowsArgs<Rule>), hipStream_t stream) {
    GdRowsArgs<Rule> r{};
    const int state_bytes = Rule::lds_floats(pad16(m.n)) * 4;
    int rows_bytes = 0;
    if (const int per_wg = rows_per_wg(m, batch, state_bytes, r.lay, rows_bytes)) {
        r.a = a;
        r.per_wg = per_wg;
        r.state_off = rows_bytes / 4;
        return launch_kernel(rows_kernel, dim3((batch + per_wg - 1) / per_wg), dim3(RTHREADS), rows_bytes + per_wg * state_bytes,
                             stream, r);
    }
    if (tile_lds > LDS_BYTES) return hipErrorNotSupported;
    return launch_kernel(tile_kernel, dim3((batch + a.fa.tile_rows - 1) / a.fa.tile_rows), dim3(NTHREADS), tile_lds, stream, a);
}

}  // namespace
}  // namespace icnn_be
