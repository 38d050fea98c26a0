// Shape checks, packed-weight layout and evaluation layout of the FICNN (included by be_ficnn.hip and be_train_ficnn.hip).
//   a_i = c_i + y Wy_i + z_{i-1} Wz_i,  z_i = relu(a_i)  (i < L);   E = sum_k z_{L-1,k} (head SUM) or a_L (head LINEAR)
// with c_i = x Wx_i + b_i the x-only context and [Wx_i ; Wy_i] = 'z_x{i}/W' (synthetic-cls/icnn.py:213-234).
// The MFMA operand layout, tile and LDS pitch rules are the FC-PICNN's (be_picnn_fc_dev.h), whose helpers are reused as
// they are.
#pragma once
#include <climits>

#include "be_picnn_fc_dev.h"

namespace icnn_be {

namespace {

inline size_t ficnn_align(size_t v) { return (v + 63) & ~(size_t)63; }     // 256-byte alignment of every pack part

// Where everything sits in wpack (floats):
//   wx [n_features][ctx_width] and bx [ctx_width]: the x rows and biases of the layers the head evaluates, column-wise
//   per hidden layer i < L: yf (Wy_i, forward operand), yb (Wy_i^T), zf (Wz_i, i > 0), zb (Wz_i^T, i > 0), MFMA fragments
//   head LINEAR: yL [n], zL [width[L-1]] plain vectors
struct FicnnPack {
    int L, ctx_width, evald;              // evald: layers the head evaluates (L or L + 1)
    int c_off[ICNN_BE_MAX_LAYERS];
    long long wx, bx, yL, zL;
    long long yf[ICNN_BE_MAX_LAYERS], yb[ICNN_BE_MAX_LAYERS], zf[ICNN_BE_MAX_LAYERS], zb[ICNN_BE_MAX_LAYERS];
    size_t total;
};

inline FicnnPack ficnn_pack_offsets(const icnn_be_ficnn_model &m) {
    FicnnPack o{};
    o.L = m.n_layers - 1;
    o.evald = m.head == ICNN_BE_FICNN_HEAD_LINEAR ? o.L + 1 : o.L;
    int c = 0;
    for (int i = 0; i < o.evald; ++i) { o.c_off[i] = c; c += m.width[i]; }
    o.ctx_width = c;
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t p = at; at += ficnn_align(floats); return (long long)p; };
    o.wx = take((size_t)m.n_features * c);
    o.bx = take((size_t)c);
    for (int i = 0; i < o.L; ++i) {
        o.yf[i] = take(packed_floats(m.n, m.width[i]));
        o.yb[i] = take(packed_floats(m.width[i], m.n));
        if (i > 0) {
            o.zf[i] = take(packed_floats(m.width[i - 1], m.width[i]));
            o.zb[i] = take(packed_floats(m.width[i], m.width[i - 1]));
        }
    }
    o.yL = o.zL = -1;
    if (o.evald > o.L) {
        o.yL = take((size_t)pad16(m.n));
        o.zL = take((size_t)pad16(m.width[o.L - 1]));
    }
    o.total = at;
    return o;
}

// LDS of one evaluation tile (floats): y | dE/dy | z_0 .. z_{L-1} | delta_{L-1}
struct FicnnLds {
    int ldY, ybuf, gbuf, dl, z_off[ICNN_BE_MAX_LAYERS], z_ld[ICNN_BE_MAX_LAYERS], floats;
};
inline FicnnLds ficnn_lds(const icnn_be_ficnn_model &m) {
    FicnnLds l{};
    const int L = m.n_layers - 1;
    int o = 0;
    l.ldY = lds_pitch(m.n);
    l.ybuf = o; o += TM * l.ldY;
    l.gbuf = o; o += TM * l.ldY;
    for (int i = 0; i < L; ++i) {
        l.z_ld[i] = lds_pitch(m.width[i]);
        l.z_off[i] = o; o += TM * l.z_ld[i];
    }
    l.dl = o; o += TM * l.z_ld[L - 1];
    l.floats = o;
    return l;
}

// 0, ICNN_BE_EINVAL (shape, head, ctx_width) or ICNN_BE_ELIMIT (an evaluation tile beyond the LDS, int index ranges)
inline int ficnn_check(const icnn_be_ficnn_model &m) {
    if (m.n_features < 1 || m.n < 1 || m.n_layers < 2) return ICNN_BE_EINVAL;
    if (m.n_layers > ICNN_BE_MAX_LAYERS) return ICNN_BE_ELIMIT;
    if (m.head != ICNN_BE_FICNN_HEAD_SUM && m.head != ICNN_BE_FICNN_HEAD_LINEAR) return ICNN_BE_EINVAL;
    const int L = m.n_layers - 1;
    for (int i = 0; i < L; ++i)
        if (m.width[i] < 1) return ICNN_BE_EINVAL;
    if (m.width[L] != 1) return ICNN_BE_EINVAL;
    long long c = 0;
    for (int i = 0; i < (m.head == ICNN_BE_FICNN_HEAD_LINEAR ? L + 1 : L); ++i) c += m.width[i];
    if (c != m.ctx_width) return ICNN_BE_EINVAL;
    for (int i = 0; i <= L; ++i)
        if (((long long)m.n_features + m.n) * m.width[i] > INT_MAX || (long long)m.n_features * c > INT_MAX) return ICNN_BE_ELIMIT;
    if ((long long)ficnn_lds(m).floats * 4 > LDS_BYTES) return ICNN_BE_ELIMIT;
    return 0;
}

}  // namespace
}  // namespace icnn_be
