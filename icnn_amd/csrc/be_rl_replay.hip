// The RL agent's replay memory on the device (RL/src/replay_memory.py; include/icnn_be.h, icnn_be_replay_enqueue and
// icnn_be_replay_sample): the arrays, the cursor, the fill and the draw counter live in device memory, so
// that a captured [sample, critic step] x iter reads the current values on every replay.
//
//   replay_enqueue_kernel   one transition from the staging row into slot i, then i <- (i + 1) % size and
//                           n <- min(size - 1, n + 1) (replay_memory.py:27-34).  One wave: it runs once per environment step.
//   replay_sample_kernel    a minibatch in one launch, one wave per sample.  The rejection loop of replay_memory.py:36-46 is
//                           wave-uniform (every lane computes the same Philox4x32-10 word) and bounded at
//                           ICNN_BE_REPLAY_MAX_ATTEMPTS; the lanes then copy the rows idx and idx + 1 (:48-52), dword by
//                           dword -- a row starts at idx * dimO * 4 bytes, which is 16-byte aligned only when dimO % 4 == 0.
//                           The last workgroup to take a ticket advances the draw counter and re-arms the ticket: every
//                           workgroup has read the counter before it takes its ticket, which a plain store by workgroup 0
//                           would not wait for.
//   vec_replay_enqueue_kernel / vec_replay_sample_kernel   the memory of E environments that step in lockstep (icnn_be_vec_replay,
//                           DESIGN.md §29): arrays [T][E][...], cursor and fill count time rows, so each of the E columns is
//                           the memory above.  The enqueue reads device buffers only (capturable); the sampler draws a time
//                           row as above and an environment with the domain tag 2, and gathers (c, e) and (c + 1, e).
//   explore_kernel          Ornstein-Uhlenbeck noise and the clip of E actions in one launch (icnn_be_explore): the normal
//                           deviates from Philox4x32-10 at (step, e, j, 3) by Box-Muller in float64, the step counter in device
//                           memory.
//
// The candidate range is clamped to the arrays from the device's own n (2 <= n <= size - 1 gives cand <= size - 3 and
// cand + 1 <= size - 2), so the gather stays inside the arrays whatever the control block holds.
#include "be_api_check.h"
#include "be_kernels.h"

namespace icnn_be {

namespace {

constexpr int ENQ_THREADS = 64;
constexpr int SMP_WAVES = 4;
constexpr int SMP_THREADS = 64 * SMP_WAVES;
enum { CTRL_I = 0, CTRL_N = 1, CTRL_DRAWS = 2, CTRL_STATUS = 3, CTRL_TICKET = 4 };

__device__ __forceinline__ int ctrl_load(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// word 0 of Philox4x32-10 (Salmon et al., SC'11) at counter (c0, c1, c2, c3) and key (k0, k1)
__device__ __forceinline__ unsigned philox4x32_10_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                        unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// all four words
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__global__ __launch_bounds__(ENQ_THREADS) void replay_enqueue_kernel(icnn_be_replay m, const unsigned char *stage) {
    const int tid = threadIdx.x;
    const int i = ctrl_load(m.ctrl + CTRL_I), n = ctrl_load(m.ctrl + CTRL_N);
    if (i < 0 || i >= m.size) {                                    // never with a control block this library wrote
        if (tid == 0) __hip_atomic_fetch_or(m.ctrl + CTRL_STATUS, ICNN_BE_REPLAY_ST_STATE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const double *s_act = reinterpret_cast<const double *>(stage);
    const float *s_obs = reinterpret_cast<const float *>(stage + 8 * (size_t)m.dimA);
    float *obs = m.observations + (long long)i * m.dimO;
    float *act = m.actions + (long long)i * m.dimA;
    for (int j = tid; j < m.dimO; j += ENQ_THREADS) obs[j] = s_obs[j];
    for (int j = tid; j < m.dimA; j += ENQ_THREADS) act[j] = (float)s_act[j];    // the reference's actions array is float32
    __syncthreads();
    if (tid == 0) {
        m.rewards[i] = s_obs[m.dimO];
        m.terminals[i] = reinterpret_cast<const unsigned *>(s_obs + m.dimO + 1)[0] != 0u;
        const int next = i + 1 == m.size ? 0 : i + 1;
        __hip_atomic_store(m.ctrl + CTRL_I, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(m.ctrl + CTRL_N, n + 1 < m.size - 1 ? n + 1 : m.size - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct SampleArgs {
    icnn_be_replay m;
    int batch;
    unsigned k0, k1;
    float *obs;
    double *act;
    float *rew;
    float *ob2;
    unsigned char *term;
    int *idx;
};

__global__ __launch_bounds__(SMP_THREADS) void replay_sample_kernel(SampleArgs a) {
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * SMP_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int cur = __builtin_amdgcn_readfirstlane(ctrl_load(a.m.ctrl + CTRL_I));
    const int n_dev = __builtin_amdgcn_readfirstlane(ctrl_load(a.m.ctrl + CTRL_N));
    const unsigned draws = (unsigned)__builtin_amdgcn_readfirstlane(ctrl_load(a.m.ctrl + CTRL_DRAWS));
    if (k < a.batch) {
        const int n = n_dev < 2 ? 2 : n_dev > a.m.size - 1 ? a.m.size - 1 : n_dev;
        const unsigned range = (unsigned)(n - 1);                  // randint(0, n - 1): uniform on [0, n - 2]
        int cand = 0;
        bool ok = false;
        for (int attempt = 0; attempt < ICNN_BE_REPLAY_MAX_ATTEMPTS && !ok; ++attempt) {
            const unsigned w = philox4x32_10_word0(draws, (unsigned)k, (unsigned)attempt, 0u, a.k0, a.k1);
            cand = (int)__umulhi(w, range);
            ok = cand != cur && a.m.terminals[cand] == 0;
        }
        if (lane == 0) {
            const int st = (ok ? 0 : ICNN_BE_REPLAY_ST_EXHAUSTED) | (n == n_dev ? 0 : ICNN_BE_REPLAY_ST_STATE);
            if (st) __hip_atomic_fetch_or(a.m.ctrl + CTRL_STATUS, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.rew[k] = a.m.rewards[cand];
            a.term[k] = a.m.terminals[cand + 1];
            a.idx[k] = cand;
        }
        const long long dimO = a.m.dimO, dimA = a.m.dimA;
        const float *src = a.m.observations + (long long)cand * dimO;     // rows cand and cand + 1 are adjacent
        float *o1 = a.obs + (long long)k * dimO, *o2 = a.ob2 + (long long)k * dimO;
        for (long long j = lane; j < dimO; j += 64) {
            o1[j] = src[j];
            o2[j] = src[dimO + j];
        }
        const float *sa = a.m.actions + (long long)cand * dimA;
        double *da = a.act + (long long)k * dimA;
        for (long long j = lane; j < dimA; j += 64) da[j] = (double)sa[j];
    }
    // the draw counter: the last workgroup to arrive advances it and re-arms the ticket for the next launch
    __syncthreads();
    if (threadIdx.x == 0) {
        const int ticket = __hip_atomic_fetch_add(a.m.ctrl + CTRL_TICKET, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == (int)gridDim.x - 1) {
            __hip_atomic_store(a.m.ctrl + CTRL_DRAWS, (int)(draws + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.m.ctrl + CTRL_TICKET, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- the memory of E lockstep environments -------------------------------------------------------------------------------

constexpr int VENQ_THREADS = 1024;        // ONE workgroup: every thread has read the cursor before thread 0 advances it

__global__ __launch_bounds__(VENQ_THREADS) void vec_replay_enqueue_kernel(icnn_be_vec_replay m, const float *obs, const double *act,
                                                                          const float *rew, const unsigned char *term) {
    const int tid = threadIdx.x;
    const int i = ctrl_load(m.ctrl + CTRL_I), n = ctrl_load(m.ctrl + CTRL_N);
    if (i < 0 || i >= m.steps) {
        if (tid == 0) __hip_atomic_fetch_or(m.ctrl + CTRL_STATUS, ICNN_BE_REPLAY_ST_STATE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const long long E = m.n_envs, no = E * m.dimO, na = E * m.dimA;
    float *d_obs = m.observations + (long long)i * no;
    float *d_act = m.actions + (long long)i * na;
    for (long long j = tid; j < no; j += VENQ_THREADS) d_obs[j] = obs[j];
    for (long long j = tid; j < na; j += VENQ_THREADS) d_act[j] = (float)act[j];
    for (long long e = tid; e < E; e += VENQ_THREADS) {
        m.rewards[(long long)i * E + e] = rew[e];
        m.terminals[(long long)i * E + e] = term[e] != 0;
    }
    __syncthreads();
    if (tid == 0) {
        const int next = i + 1 == m.steps ? 0 : i + 1;
        __hip_atomic_store(m.ctrl + CTRL_I, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(m.ctrl + CTRL_N, n + 1 < m.steps - 1 ? n + 1 : m.steps - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct VecSampleArgs {
    icnn_be_vec_replay m;
    int batch;
    unsigned k0, k1;
    float *obs;
    double *act;
    float *rew;
    float *ob2;
    unsigned char *term;
    int *idx;
};

__global__ __launch_bounds__(SMP_THREADS) void vec_replay_sample_kernel(VecSampleArgs a) {
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * SMP_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int cur = __builtin_amdgcn_readfirstlane(ctrl_load(a.m.ctrl + CTRL_I));
    const int n_dev = __builtin_amdgcn_readfirstlane(ctrl_load(a.m.ctrl + CTRL_N));
    const unsigned draws = (unsigned)__builtin_amdgcn_readfirstlane(ctrl_load(a.m.ctrl + CTRL_DRAWS));
    if (k < a.batch) {
        const int n = n_dev < 2 ? 2 : n_dev > a.m.steps - 1 ? a.m.steps - 1 : n_dev;
        const unsigned range = (unsigned)(n - 1);
        const long long E = a.m.n_envs;
        int cand = 0, env = 0;
        bool ok = false;
        for (int attempt = 0; attempt < ICNN_BE_REPLAY_MAX_ATTEMPTS && !ok; ++attempt) {
            const unsigned w0 = philox4x32_10_word0(draws, (unsigned)k, (unsigned)attempt, 0u, a.k0, a.k1);
            const unsigned w2 = philox4x32_10_word0(draws, (unsigned)k, (unsigned)attempt, 2u, a.k0, a.k1);
            cand = (int)__umulhi(w0, range);
            env = (int)__umulhi(w2, (unsigned)a.m.n_envs);
            ok = cand != cur && a.m.terminals[cand * E + env] == 0;
        }
        const long long at = cand * E + env;                       // (c, e); its successor (c + 1, e) lies E entries on
        if (lane == 0) {
            const int st = (ok ? 0 : ICNN_BE_REPLAY_ST_EXHAUSTED) | (n == n_dev ? 0 : ICNN_BE_REPLAY_ST_STATE);
            if (st) __hip_atomic_fetch_or(a.m.ctrl + CTRL_STATUS, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.rew[k] = a.m.rewards[at];
            a.term[k] = a.m.terminals[at + E];
            a.idx[k] = (int)at;
        }
        const long long dimO = a.m.dimO, dimA = a.m.dimA;
        const float *src = a.m.observations + at * dimO;
        float *o1 = a.obs + (long long)k * dimO, *o2 = a.ob2 + (long long)k * dimO;
        for (long long j = lane; j < dimO; j += 64) {
            o1[j] = src[j];
            o2[j] = src[E * dimO + j];
        }
        const float *sa = a.m.actions + at * dimA;
        double *da = a.act + (long long)k * dimA;
        for (long long j = lane; j < dimA; j += 64) da[j] = (double)sa[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int ticket = __hip_atomic_fetch_add(a.m.ctrl + CTRL_TICKET, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == (int)gridDim.x - 1) {
            __hip_atomic_store(a.m.ctrl + CTRL_DRAWS, (int)(draws + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.m.ctrl + CTRL_TICKET, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- exploration ------------------------------------------------------------------------------------------------------------

constexpr int EXP_THREADS = 256;          // ONE workgroup: every thread has read the step counter before thread 0 advances it

struct ExploreArgs {
    int count;                            // E * dimA
    int dimA, raw_f32, test;
    const void *raw;
    double *noise, *action;
    int *counter;
    double theta, sigma;
    unsigned k0, k1;
};

__global__ __launch_bounds__(EXP_THREADS) void explore_kernel(ExploreArgs a) {
#pragma clang fp contract(off)
    const unsigned step = (unsigned)ctrl_load(a.counter);
    for (int t = threadIdx.x; t < a.count; t += EXP_THREADS) {
        double x = a.raw_f32 ? (double)static_cast<const float *>(a.raw)[t] : static_cast<const double *>(a.raw)[t];
        if (!a.test) {
            unsigned w[4];
            philox4x32_10(step, (unsigned)(t / a.dimA), (unsigned)(t % a.dimA), 3u, a.k0, a.k1, w);
            // 53 bits each: u1 in (0, 1] for the logarithm, u2 in [0, 1)
            const unsigned long long b1 = (((unsigned long long)w[1] << 32) | w[0]) >> 11;
            const unsigned long long b2 = (((unsigned long long)w[3] << 32) | w[2]) >> 11;
            const double u1 = (double)(b1 + 1ull) * 0x1p-53, u2 = (double)b2 * 0x1p-53;
            const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
            double nz = a.noise[t];
            nz = nz - (a.theta * nz - a.sigma * z);
            a.noise[t] = nz;
            x = x + nz;
        }
        a.action[t] = fmin(fmax(x, -1.0), 1.0);
    }
    __syncthreads();
    if (threadIdx.x == 0 && !a.test) __hip_atomic_store(a.counter, (int)(step + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

unsigned sample_blocks(int batch) { return (unsigned)(((long long)batch + SMP_WAVES - 1) / SMP_WAVES); }

// what icnn_be_replay_enqueue and icnn_be_replay_sample refuse in the memory's descriptor
int check_replay(const icnn_be_replay *m) {
    if (!m || m->size < 3 || m->dimO < 1 || m->dimA < 1) return ICNN_BE_EINVAL;
    if (misaligned(m->observations, 4) || misaligned(m->actions, 4) || misaligned(m->rewards, 4) || !m->terminals ||
        misaligned(m->ctrl, 4))
        return ICNN_BE_EINVAL;
    return 0;
}

// the same for the memory of E lockstep environments; idx = c * E + e is an int
int check_vec_replay(const icnn_be_vec_replay *m) {
    if (!m || m->steps < 3 || m->n_envs < 1 || m->dimO < 1 || m->dimA < 1) return ICNN_BE_EINVAL;
    if ((long long)m->steps * m->n_envs > 0x7fffffffLL) return ICNN_BE_ELIMIT;
    if (misaligned(m->observations, 4) || misaligned(m->actions, 4) || misaligned(m->rewards, 4) || !m->terminals ||
        misaligned(m->ctrl, 4))
        return ICNN_BE_EINVAL;
    return 0;
}

// a minibatch drawn from `slots` transitions of which `fill` are written: what both sample entries refuse, then the
// arguments their kernels share
template <typename Args>
int sample_args(Args &a, int slots, int fill, int batch, unsigned long long seed, float *obs, double *act, float *rew,
                float *ob2, unsigned char *term, int *idx, void *stream) {
    if (batch < 1 || fill < 2 || fill > slots - 1) return ICNN_BE_EINVAL;
    if (misaligned(obs, 4) || misaligned(act, 8) || misaligned(rew, 4) || misaligned(ob2, 4) || !term || misaligned(idx, 4) ||
        !stream_ok(stream))
        return ICNN_BE_EINVAL;
    a.batch = batch;
    a.k0 = (unsigned)(seed & 0xffffffffull);
    a.k1 = (unsigned)(seed >> 32);
    a.obs = obs;
    a.act = act;
    a.rew = rew;
    a.ob2 = ob2;
    a.term = term;
    a.idx = idx;
    return 0;
}

}  // namespace
}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_replay_enqueue(const icnn_be_replay *m, const void *stage, void *stream) {
    if (int rc = check_replay(m)) return rc;
    if (misaligned(stage, 8) || !stream_ok(stream)) return ICNN_BE_EINVAL;
    return api_done(launch_kernel(replay_enqueue_kernel, dim3(1), dim3(ENQ_THREADS), 0, static_cast<hipStream_t>(stream), *m,
                                  static_cast<const unsigned char *>(stage)));
}

int icnn_be_replay_sample(const icnn_be_replay *m, int fill, int batch, unsigned long long seed, float *obs, double *act,
                          float *rew, float *ob2, unsigned char *term, int *idx, void *stream) {
    if (int rc = check_replay(m)) return rc;
    SampleArgs a{};
    if (int rc = sample_args(a, m->size, fill, batch, seed, obs, act, rew, ob2, term, idx, stream)) return rc;
    a.m = *m;
    return api_done(launch_kernel(replay_sample_kernel, dim3(sample_blocks(batch)), dim3(SMP_THREADS), 0,
                                  static_cast<hipStream_t>(stream), a));
}

int icnn_be_vec_replay_enqueue(const icnn_be_vec_replay *m, const float *obs, const double *act, const float *rew,
                               const unsigned char *term, void *stream) {
    if (int rc = check_vec_replay(m)) return rc;
    if (misaligned(obs, 4) || misaligned(act, 8) || misaligned(rew, 4) || !term || !stream_ok(stream)) return ICNN_BE_EINVAL;
    return api_done(launch_kernel(vec_replay_enqueue_kernel, dim3(1), dim3(VENQ_THREADS), 0, static_cast<hipStream_t>(stream), *m,
                                  obs, act, rew, term));
}

int icnn_be_vec_replay_sample(const icnn_be_vec_replay *m, int fill, int batch, unsigned long long seed, float *obs, double *act,
                              float *rew, float *ob2, unsigned char *term, int *idx, void *stream) {
    if (int rc = check_vec_replay(m)) return rc;
    VecSampleArgs a{};
    if (int rc = sample_args(a, m->steps, fill, batch, seed, obs, act, rew, ob2, term, idx, stream)) return rc;
    a.m = *m;
    return api_done(launch_kernel(vec_replay_sample_kernel, dim3(sample_blocks(batch)), dim3(SMP_THREADS), 0,
                                  static_cast<hipStream_t>(stream), a));
}

int icnn_be_explore(int n_envs, int dimA, const void *raw, int raw_f32, double *noise, int *counter, double theta, double sigma,
                    unsigned long long seed, int test, double *action, void *stream) {
    if (n_envs < 1 || dimA < 1 || !raw || !noise || !counter || !action) return ICNN_BE_EINVAL;
    if ((long long)n_envs * dimA > 0x7fffffffLL) return ICNN_BE_ELIMIT;
    if (!(theta == theta) || !(sigma == sigma)) return ICNN_BE_EINVAL;
    if (misaligned(raw, raw_f32 ? 4 : 8) || misaligned(noise, 8) || misaligned(action, 8) || misaligned(counter, 4) ||
        !stream_ok(stream))
        return ICNN_BE_EINVAL;
    ExploreArgs a{};
    a.count = n_envs * dimA;
    a.dimA = dimA; a.raw_f32 = raw_f32 != 0; a.test = test != 0;
    a.raw = raw; a.noise = noise; a.action = action; a.counter = counter;
    a.theta = theta; a.sigma = sigma;
    a.k0 = (unsigned)(seed & 0xffffffffull);
    a.k1 = (unsigned)(seed >> 32);
    return api_done(launch_kernel(explore_kernel, dim3(1), dim3(EXP_THREADS), 0, static_cast<hipStream_t>(stream), a));
}

}  // extern "C"
