// Persistent per-tile solve of a fully-connected PICNN: one workgroup owns a tile of 16 samples for ALL rounds
// of the bundle-entropy loop and alternates the two phases in place,
//     phase A  fc_fg_tile     (16 waves: the MFMA chain of be_picnn_fc_dev.h, energy + gradient of the tile)
//     phase B  dual_step_body (one wave per sample: cut, rank test, projected Newton, y update)
// Both kernels are latency chains -- fc_fg takes as long for one tile as for 256, a dual step as long as its
// slowest sample -- so with one launch per phase every sample waited for the slowest of the whole batch ten times
// per solve (about 15 Newton updates when the mean is 3.8).  Here a tile only waits for the slowest of ITS
// sixteen samples, and there is a single launch.  The arithmetic is exactly that of the two-kernel path (same
// device functions), so the results are bit-identical (tests/test_gpu_parity.py).
//
// LDS is shared in time: phase A uses its activation buffers, phase B the 16 staged bundles plus one shared
// pair of constant rows (zeros / ones for the MFMA operand masking); each phase re-initialises what it needs.
#include "be_dual_dev.h"
#include "be_dual_small_dev.h"
#include "be_picnn_fc_dev.h"
#include "be_picnn_fc_rows_dev.h"

namespace icnn_be {

namespace {

static_assert(NWAVE == TM, "one wave per sample in the dual phase");

// Round class of the Bibsonomy headline instance (fused_fc_solve_kernel, CLASSES): rounds 0 .. 7, whose bundles hold at most
// eight cuts, run the dual body compiled for that cap.  One class: bodies for up to 4 and up to 6 cuts on top of it measured
// within the noise of this one (profiles/round_classes_ab.md) and are not in the tree.
constexpr int ROUND_CLASS_CAP = HV_K1MAX;

// One kernel parameter, read through the kernel-argument segment (s_load) by both phases.
//
// Both phases are INLINED into the round loop.  As non-inlined functions (round 1) each of them saved and restored
// the 44 callee-saved VGPRs it uses on every call: 239 dwords per lane, round and wave = 2.5 GB of scratch traffic
// per solve of 4096 samples, three times the algorithmic bytes (profiles/r02_a_pmc.md).  Inlined naively they
// spilled instead, for a reason that has nothing to do with their own register need: everything derived from
// threadIdx.x (lane, wave, fragment coordinates, LDS offsets) and every literal (the double-precision polynomial
// coefficients of exp) is invariant in the round loop, gets hoisted in front of it -- IR-level LICM for the
// former, MachineLICM for the latter -- and, each phase needing the whole 128-register budget, is then spilled
// and reloaded at every use.  Two measures make the inlined kernel spill-free (0 scratch loads/stores, 127 VGPRs):
// the thread index is read through an opaque move (thread_id(), be_common.h), and this translation unit is
// compiled with -mllvm -disable-machine-licm (icnn_amd/build.py), so literals are materialised where they are used.
struct FusedArgs {
    DualArgs da;       // first: dual_step_body re-reads it at offset 0 of the kernel-argument segment
    FcArgs fa;
    int rounds, crow_off, samples_off, sample_bytes;
    int grouped;       // 1: the sixteen staged bundles of a round do not fit the LDS together (more than ~10 cuts per
                       // sample at n = 159): every round the live samples are dealt into groups whose bundles do fit --
                       // each sample sized for the cuts it holds NOW, finished samples for nothing -- and the groups run
                       // the dual phase one after the other (group_cap = bytes of the staging region, need_off = a
                       // [TM] int array behind the constant rows)
    int group_cap, need_off;
    long long *trace;  // diagnostic (profiling build, icnn_be_debug_trace): [B][ICNN_BE_MAX_ITERS][DUAL_TRACE_WORDS] or null
    SolveReset reset;  // on: the state is reset in front of round 0 (reset_sample)
};
typedef const __attribute__((address_space(4))) FusedArgs KArgs;

// The reset of a solve inside its first launch: what the caller's y <- y0 and state_init_kernel (be_dual.hip) write for sample
// u, written by the wave that owns the sample for the whole solve.  st.pending is left alone: only the launch rounds of the
// other plans write it.  The caller's barrier (with its workgroup-scope release) makes the words visible to the other waves of
// the workgroup; no other workgroup ever reads them.
__device__ __forceinline__ void reset_sample(const icnn_be_state &st, const SolveReset &rs, int u, int lane) {
    const int n = st.n;
    double *yr = st.y + (size_t)u * n;
    if (rs.y0) {
        const double *src = rs.y0 + (size_t)u * n;
        for (int j = lane; j < n; j += 64) yr[j] = src[j];
    } else {
        for (int j = lane; j < n; j += 64) yr[j] = rs.fill;
    }
    if (lane == 0) {
        st.count[u] = 0;
        st.finished[u] = 0;
        st.status[u] = 0;
        st.n_iters[u] = st.iters > 0 ? st.iters : st.slots;
        st.newton_iters[u] = 0;
        st.t_next[u] = 0;
        st.phase[u] = 0;
        st.skip_fg[u] = 0;
    }
}

// RL: the variant of RL/src/bundle_entropy.py (clipped y, Armijo search, early stop); IPM: the interior-point variant of
// lib/bundle_entropy.py (round 4: the module the reference's scripts import runs through the persistent kernels as well)
// SLICED: the budgeted form (ICNN_BE_FLAG_PERSISTENT | ICNN_BE_FLAG_TIME_SLICE, variant dual): samples may be parked
// Shape (be_kernels.h): DynShape, or a FixedShape instance the launcher takes when -- and only when -- model and state match it
// (pick_shape_instance below): n, the widths and everything that follows from them are constants of the instance.
// GROUPED: -1 = args.grouped decides at run time; 0 / 1 = the launcher's layout decision is the instance's, and the dual body of
// the other form is not compiled in.
// CLASSES (with GROUPED = 0, KT = 16, variant dual on the fused VALU pass): rows_cap = round + 1 is wave-uniform and known from
// the round alone, so the rounds whose bundles hold at most ROUND_CLASS_CAP cuts run a dual body compiled for that cap
// (dual_step_body, KCAP): no function call in its Newton loop, no MFMA sweep compiled in.  Later rounds run the body as it is.
template <bool RL, int KT, bool IPM = false, bool SLICED = false, typename Shape = DynShape, int GROUPED = -1, bool CLASSES = false>
__global__ __launch_bounds__(NTHREADS) void fused_fc_solve_kernel(FusedArgs args) {
    static_assert(!CLASSES || (GROUPED == 0 && KT == 16 && !RL && !IPM && !SLICED), "round classes: the ungrouped 16-slot dual instance");
    using Wave = DualCfg<float, KT, 1, RL, IPM>;                    // phase B: one wave per sample
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    KArgs *kp0 = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    {
        const int ldA = Shape::ldA(args.da);
        float *crow = reinterpret_cast<float *>(smem + args.crow_off);  // behind phase A's buffers: written once
        for (int j = thread_id(); j < 2 * ldA; j += NTHREADS) crow[j] = j < ldA ? 0.f : 1.f;
        if ((GROUPED < 0 ? args.grouped != 0 : GROUPED != 0) && thread_id() < TM)
            reinterpret_cast<int *>(smem + args.need_off)[TM + thread_id()] = 0;   // done flags
    }
    if (args.reset.on) {                                            // wave w owns sample w of the tile
        const int wave = uni(thread_id() >> 6), u = blockIdx.x * args.fa.tile_rows + wave;
        if (wave < args.fa.tile_rows && u < args.da.st.batch) reset_sample(args.da.st, args.reset, u, thread_id() & 63);
        __syncthreads();                                            // phase A reads the skip flags of the tile on wave 0
    }
    const int rounds = args.rounds;
    for (int r = 0; r < rounds; ++r) {
        KArgs *kp = kp0;
        int tile = blockIdx.x;
        asm volatile("" : "+s"(kp), "+s"(tile));                    // nothing derived from the arguments is carried
        fc_fg_tile<Shape>(kp->fa, tile, reinterpret_cast<float *>(smem));  // phase A: f, g of the tile -> global work arrays
        __syncthreads();                                            // ... visible to the tile's dual waves
        int wave = uni(thread_id() >> 6), round = r;
        asm volatile("" : "+s"(kp), "+s"(tile), "+s"(wave), "+s"(round));
        KArgs &k = *kp;
        const int u = tile * k.fa.tile_rows + wave;
        const bool mine = wave < k.fa.tile_rows && u < k.da.st.batch;
        if (GROUPED < 0 ? !k.grouped : GROUPED == 0) {
            if (mine) {                                             // phase B: wave w = sample w of the tile
                const int rows_cap = round + 1 < k.da.st.slots ? round + 1 : k.da.st.slots;
                unsigned char *region = smem + k.samples_off + wave * k.sample_bytes;
                const float *crow = reinterpret_cast<const float *>(smem + k.crow_off);
                if (CLASSES && round < ROUND_CLASS_CAP)             // rows_cap <= round + 1 <= the cap of the class
                    dual_step_body<DualCfgTile<Wave, SLICED, Shape, CLASSES ? ROUND_CLASS_CAP : 0>>(k.da, u, thread_id() & 63, region, round, rows_cap, crow);
                else
                    dual_step_body<DualCfgTile<Wave, SLICED, Shape>>(k.da, u, thread_id() & 63, region, round, rows_cap, crow);
            }
            __syncthreads();                                        // y, skip flags visible to the next phase A
            continue;
        }
        // phase B in groups: what a sample needs this round follows from the cuts it holds (count + the new one)
        int *need = reinterpret_cast<int *>(smem + k.need_off);
        int kk = 0;
        if (mine && k.da.st.finished[u] == 0 && k.da.st.t_next[u] < k.rounds) kk = k.da.st.count[u] + 1;
        kk = uni(kk);
        // never more rows than the sample has slots: with every slot active and one more cut to take (iterations beyond the
        // slot count recycle the slots of PRUNED cuts only) the dual step must see k > rows_cap and report ICNN_BE_ST_OVERFLOW,
        // as the launch pairs and the per-sample kernel do, instead of writing a 32nd row behind the sample's arrays
        if (kk > k.da.st.slots) kk = k.da.st.slots;
        if ((thread_id() & 63) == 0)
            need[wave] = kk > 0 ? (carve(KT, kk, Shape::ldA(k.da), Shape::n_pad(k.da), 4, Shape::plan(k.da).n_leaves, RL, 1, false, IPM).total + 15) & ~15 : 0;
        __syncthreads();
        // (Round 6, tried and withdrawn: dealing the regions longest-first by the Newton updates of the sample's previous dual
        //  step.  The sample that ends a round is not predictable from its last round -- rank 10 of 16 on average,
        //  profiles/r06_c4_trace_longest_first.txt --, the deal moved the queueing around without shortening a tile's dual phase: 6.51 -> 6.55 ms.)
        int g = 0, off = 0, my_g = 0, my_off = 0;
        for (int i = 0; i < TM; ++i) {                              // the same greedy deal in every wave
            const int nb = need[i];
            if (off + nb > k.group_cap) { ++g; off = 0; }
            if (i == wave) { my_g = g; my_off = off; }
            off += nb;
        }
        my_g = uni(my_g); my_off = uni(my_off);
        int alive = kk > 0;
        // The groups do not wait for each other as groups: a sample of a later group starts as soon as every sample of an
        // EARLIER group whose staging region overlaps its own has finished (a flag per sample, stamped with the round; only
        // waves of earlier groups are ever waited for, the first group waits for nobody: no cycle, and a finished wave's
        // flag is set on every path out of the dual step).  A tile's dual phase then lasts as long as its longest chain of
        // overlapping samples instead of the sum over groups of each group's slowest sample.
        int *done = need + TM;
        // diagnostic (profiling build): cycles this sample spends queueing for its staging region (phase 14) and, below,
        // waiting at the barrier that ends the tile's dual phase (phase 15); tools/c4_timeline.py
        long long tq = ICNN_BE_PROF_ON(k.da.prof) ? (long long)__builtin_readcyclecounter() : 0;
        auto wait_lap = [&](int phase) {
            if (ICNN_BE_PROF_ON(k.da.prof)) {
                const long long now = (long long)__builtin_readcyclecounter();
                if (mine && (thread_id() & 63) == 0)
                    atomicAdd(reinterpret_cast<unsigned long long *>(k.da.prof) + (size_t)u * DUAL_PROF_PHASES + phase,
                              (unsigned long long)(now - tq));
                tq = now;
            }
        };
        long long *tr = nullptr;
        if (ICNN_BE_PROF_ON(k.trace) && kk > 0 && (thread_id() & 63) == 0) {
            tr = k.trace + ((size_t)u * ICNN_BE_MAX_ITERS + round) * DUAL_TRACE_WORDS;
            tr[0] = tq; tr[3] = k.da.st.newton_iters[u];
        }
        if (kk > 0) {
            if (my_g > 0) {
                const int my_end = my_off + need[wave];
                int gi = 0, oi = 0;
                for (int i = 0; i < TM; ++i) {
                    const int nb = need[i];
                    if (oi + nb > k.group_cap) { ++gi; oi = 0; }
                    if (gi >= my_g) break;
                    if (nb > 0 && oi < my_end && oi + nb > my_off)
                        while (__atomic_load_n(&done[i], __ATOMIC_RELAXED) != round + 1) __builtin_amdgcn_s_sleep(4);
                    oi += nb;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            wait_lap(14);
            if (ICNN_BE_PROF_ON(k.trace) && tr) tr[1] = (long long)__builtin_readcyclecounter();
            dual_step_body<DualCfgTile<Wave, SLICED, Shape>>(k.da, u, thread_id() & 63, smem + k.samples_off + my_off, round, kk,
                                                             reinterpret_cast<const float *>(smem + k.crow_off));
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // its LDS traffic is complete before the flag is seen
            if ((thread_id() & 63) == 0) __atomic_store_n(&done[wave], round + 1, __ATOMIC_RELAXED);
            if (ICNN_BE_PROF_ON(k.da.prof)) tq = (long long)__builtin_readcyclecounter();
            if (ICNN_BE_PROF_ON(k.trace) && tr) tr[2] = (long long)__builtin_readcyclecounter();
        }
        const int any_alive = __syncthreads_or(alive);
        if (kk > 0) wait_lap(15);
        if (!any_alive) break;                        // (also the barrier that ends the dual phase) no sample
                                                                    // of the tile has work left: none gets any later either
    }
}

// ---------------------------------------------------------------------------------------------------------
// Batches of at most one sample per CU: a persistent workgroup PER SAMPLE (8 waves).  Phase A is the VALU
// evaluation of be_picnn_fc_rows_dev.h (all waves), phase B the dual step of the sample on wave 0; the context
// row and the iteration-invariant products stay in LDS for the whole solve, both phases have their own LDS
// regions.  Besides the single launch, every sample now runs at its own pace: the solve ends with the sample
// whose ten rounds are longest in SUM, not with the sum over rounds of the slowest sample of each round, and a
// sample that leaves the loop (rank test, RL stall) frees its CU at once.  Same device functions, same bits.
// ---------------------------------------------------------------------------------------------------------
struct FusedRowsArgs {
    DualArgs da;       // first: dual_step_body re-reads it at offset 0 of the kernel-argument segment
    FcArgs fa;
    RowsLayout lay;
    int rounds, per_wg;                // samples per workgroup (1 or 2)
    int dual_off, sample_bytes, crow_off;    // byte offsets of the dual steps' regions and of the constant rows
    int iters;                         // outer iterations (icnn_be_state.iters, or its slots)
    int resume;                        // finishing pass after time-sliced rounds: only samples that still have rounds to
                                       // run (parked in a Newton loop or behind by the rounds they were parked in) do
                                       // anything, each from its own outer-iteration counter, with no update budget
    SolveReset reset;                  // on (never with resume): the state is reset in front of round 0 (reset_sample)
    RowsValue value;                   // VALUE kernels only (icnn_be_rl_bundle_solve): where the epilogue writes 2y - 1 and E(y)
};
typedef const __attribute__((address_space(4))) FusedRowsArgs KRArgs;

// phase A of the per-sample kernel: the VALU evaluation of be_picnn_fc_rows_dev.h on all waves
// VALUE: the same evaluation as the epilogue of icnn_be_rl_bundle_solve -- the energy goes to value.q and the action 2y - 1
// (float64, from the y the input was rounded from) to value.act; the work arrays keep what the last round left in them
template <bool VALUE = false>
__device__ __forceinline__ void rows_phase_fg(KRArgs *kp, int s_base, int batch, int tid) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    KRArgs &k = *kp;
    float *lds = reinterpret_cast<float *>(smem);
    const int wave = tid >> 6, lane = tid & 63, n = k.fa.n, RF = k.lay.row_floats;
    long long tick = ICNN_BE_PROF_ON(k.fa.prof) ? (long long)__builtin_readcyclecounter() : 0;
    auto lap = [&](int phase) {          // diagnostic only (tools/rows_phase_profile.py)
        if (ICNN_BE_PROF_ON(k.fa.prof)) {
            const long long now = (long long)__builtin_readcyclecounter();
            if (lane == 0)
                atomicAdd(reinterpret_cast<unsigned long long *>(k.fa.prof) +
                              ((size_t)blockIdx.x * RWAVES + wave) * FC_PROF_PHASES + phase,
                          (unsigned long long)(now - tick));
            tick = now;
        }
    };
    if (wave < batch)                    // network input: y rounded to float32 like a TensorFlow feed; RL wrapper feeds 2y-1
        for (int j = lane; j < n; j += 64) {
            const double yd = k.da.st.y[(size_t)(s_base + wave) * n + j];
            rows_set_input(k.fa, k.lay, lds + wave * RF, j, k.fa.action_box ? (float)(2.0 * yd - 1.0) : (float)yd);
        }
    __syncthreads();
    lap(13);
    rows_eval(k.fa, k.lay, lds, batch, tid, lap);
    if constexpr (VALUE) {
        if (wave < batch) {
            if (lane == 0 && k.value.q) k.value.q[s_base + wave] = lds[k.lay.f_off + wave];
            for (int j = lane; j < n; j += 64) {
                const size_t at = (size_t)(s_base + wave) * n + j;
                k.value.act[at] = 2.0 * k.da.st.y[at] - 1.0;
            }
        }
        return;
    }
    if (wave < batch) {                  // hand-over to the dual step of the sample (same wave) through its work arrays
        const float gscale = k.fa.action_box ? 2.f : 1.f;
        if (lane == 0) k.fa.f[s_base + wave] = lds[k.lay.f_off + wave];
        for (int j = lane; j < n; j += 64) k.fa.g[(size_t)(s_base + wave) * n + j] = gscale * lds[wave * RF + k.lay.g_off + j];
    }
    lap(14);
}

// KS > 0: narrow rows (n <= 16, variant RL): the dual steps of ALL samples of the workgroup (at most four) run on wave 0, one
// sample per 16-lane DPP row with the bundle in registers (be_dual_small_dev.h, KS = its row count) -- the RL agent's act()
// and its replay batches up to four samples per CU.  Bit-identical to the wave-per-sample phase.
// VALUE (variant RL, never a resume launch): one more evaluation of every sample of the workgroup behind the last round
// (rows_phase_fg<true>), whichever way the workgroup left the round loop.
template <bool RL, int KT, int KS = 0, bool IPM = false, bool VALUE = false>
__global__ __launch_bounds__(RTHREADS) void fused_rows_solve_kernel(FusedRowsArgs args) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int per_wg = args.per_wg;
    int s_base0 = blockIdx.x * per_wg;
    const int batch0 = args.da.st.batch - s_base0 < per_wg ? args.da.st.batch - s_base0 : per_wg;
    KRArgs *kp0 = (KRArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    if (args.resume) {                                              // nothing to do for a workgroup whose samples are done
        int todo = 0;
        if (thread_id() < batch0) {
            const int u = s_base0 + thread_id();
            todo = args.da.st.finished[u] == 0 && args.da.st.t_next[u] < args.iters;
        }
        if (!__syncthreads_or(todo)) return;
    }
    if (args.reset.on) {                                            // wave w owns sample w of the workgroup; the barriers of
        const int wave = uni(thread_id() >> 6);                     // rows_setup below publish the words to the other waves
        if (wave < batch0) reset_sample(args.da.st, args.reset, s_base0 + wave, thread_id() & 63);
    }
    {
        float *crow = reinterpret_cast<float *>(smem + args.crow_off);
        for (int j = thread_id(); j < 2 * args.da.ldA; j += RTHREADS) crow[j] = j < args.da.ldA ? 0.f : 1.f;
    }
    rows_setup(args.fa, args.lay, reinterpret_cast<float *>(smem), s_base0, batch0, thread_id());
    const int rounds = args.rounds;
    for (int r = 0; r < rounds; ++r) {
        // both phases inlined, arguments and thread index re-read opaquely per round (see fused_fc_solve_kernel)
        KRArgs *kp = kp0;
        int s_base = s_base0, batch = batch0, round = r;
        asm volatile("" : "+s"(kp), "+s"(s_base), "+s"(batch), "+s"(round));
        rows_phase_fg(kp, s_base, batch, thread_id());
        __syncthreads();                                            // f, g visible (written by the dual wave itself)
        const int wave = uni(thread_id() >> 6);
        asm volatile("" : "+s"(kp), "+s"(s_base), "+s"(batch), "+s"(round));
        KRArgs &k = *kp;
        int live = 0;                                               // (each dual wave reads the flags it wrote itself)
        if constexpr (KS > 0) {
            if (wave == 0) {
                dual_step_quad_rl<float, KS>(k.da, s_base, batch, round);
                if ((thread_id() & 63) < batch) live = k.da.st.skip_fg[s_base + (thread_id() & 63)] == 0;
            }
        } else {
            if (wave < batch) {
                const int rows_cap = !k.resume && round + 1 < k.da.st.slots ? round + 1 : k.da.st.slots;
                dual_step_body<DualCfg<float, KT, 1, RL, IPM>>(k.da, s_base + wave, thread_id() & 63, smem + k.dual_off + wave * k.sample_bytes,
                                                               round, rows_cap, reinterpret_cast<const float *>(smem + k.crow_off));
            }
            if (wave < batch && (thread_id() & 63) == 0) {
                const int u = s_base + wave;
                live = k.resume ? (k.da.st.finished[u] == 0 && k.da.st.t_next[u] < k.iters) : k.da.st.skip_fg[u] == 0;
            }
        }
        if (!__syncthreads_or(live)) break;                         // every sample of the workgroup has left the loop
    }
    if constexpr (VALUE) {
        // Both ways out of the loop pass the barrier above behind the last dual step, but with narrow rows wave 0 wrote the y
        // rows that waves 1.. now read: a full barrier, whose workgroup-scope release / acquire covers global memory.
        __syncthreads();
        KRArgs *kp = kp0;
        int s_base = s_base0, batch = batch0;
        asm volatile("" : "+s"(kp), "+s"(s_base), "+s"(batch));
        rows_phase_fg<true>(kp, s_base, batch, thread_id());
    }
}

}  // namespace

// LDS of one sample's dual step in the persistent kernels: the carve-up of a bundle that fills every slot, without constant
// rows of its own (the workgroup shares one pair)
static int sample_region_bytes(const icnn_be_state &st, int ldA, int n_pad, int n_leaves) {
    const bool rl = st.variant == ICNN_BE_VARIANT_RL, ipm = st.variant == ICNN_BE_VARIANT_PDIPM;
    return (carve(st.slots > 15 ? 32 : 16, st.slots, ldA, n_pad, 4, n_leaves, rl, 1, false, ipm).total + 15) & ~15;
}

bool fused_rows_layout(const icnn_be_fc_model &m, const icnn_be_state &st, int per_wg, bool resume, FusedRowsLayout &out) {
    const bool ipm = st.variant == ICNN_BE_VARIANT_PDIPM;
    if (st.cut_dtype != ICNN_BE_CUT_F32 || per_wg < 1 || per_wg > ROWS_MAX) return false;
    if (dual_waves(st.n, st.cut_dtype, st.variant) != 1 || (ipm && resume)) return false;
    PairwisePlan plan;
    if (!pw_build(plan, st.n)) return false;
    const int n_pad = (st.n + 15) & ~15, ldA = dual_row_pitch(n_pad);
    RowsLayout lay;
    out.dual_off = (rows_layout(m, per_wg, lay) + 15) & ~15;
    out.sample_bytes = sample_region_bytes(st, ldA, n_pad, plan.n_leaves);
    out.crow_off = out.dual_off + per_wg * out.sample_bytes;
    out.lds = out.crow_off + ((2 * ldA * 4 + 15) & ~15);
    return out.lds <= LDS_BYTES;
}

bool fused_tile_layout(const icnn_be_fc_model &m, const icnn_be_state &st, int tile_rows, int budget, FusedTileLayout &out) {
    const bool rl = st.variant == ICNN_BE_VARIANT_RL, ipm = st.variant == ICNN_BE_VARIANT_PDIPM;
    if (st.cut_dtype != ICNN_BE_CUT_F32 || (tile_rows != 4 && tile_rows != 8 && tile_rows != TM)) return false;
    if (dual_waves(st.n, st.cut_dtype, st.variant) != 1 || ((ipm || rl) && budget > 0)) return false;
    // a narrow model (icnn_be_fc_model.tile_rows 8 or 4) has no persistent tile kernel: the plan falls through to the launch
    // pairs, whose fc_fg_kernel runs the narrow tile.  (The tile kernel's own 4 / 8 sample tiles are 16-row LDS layouts.)
    if (fc_model_narrow(m)) return false;
    FcArgs fa{};
    int fg_bytes = 0;
    PairwisePlan plan;
    if (fill_args(m, fa, fg_bytes) != 0 || !pw_build(plan, st.n)) return false;
    const bool big = st.slots > 15;
    const int n_pad = (st.n + 15) & ~15, ldA = dual_row_pitch(n_pad);
    out.sample_bytes = sample_region_bytes(st, ldA, n_pad, plan.n_leaves);
    // phase B: sixteen bundles from offset 0 (they overlay phase A's buffers); the shared constant rows live behind
    // whichever region is larger, where neither phase overwrites them
    const int crow_bytes = (2 * ldA * 4 + 15) & ~15, dual_bytes = TM * out.sample_bytes;
    out.crow_off = ((fg_bytes > dual_bytes ? fg_bytes : dual_bytes) + 15) & ~15;
    out.lds = out.crow_off + crow_bytes;
    out.grouped = out.group_cap = out.need_off = 0;
    if (out.lds > LDS_BYTES || big) {
        // the sixteen full-size bundles do not fit together: groups sized by what the samples hold (FusedArgs::grouped).
        // The staging region takes everything the workgroup can have; one sample's largest bundle must fit it.
        const int need_bytes = 2 * TM * 4;            // per sample: bytes needed this round, and its done flag
        out.crow_off = (LDS_BYTES - 1024 - crow_bytes - need_bytes) & ~15;      // (1 KB: the kernel's static LDS, 256 B today)
        if (out.crow_off < fg_bytes || out.crow_off < out.sample_bytes) return false;
        out.grouped = 1; out.group_cap = out.crow_off; out.need_off = out.crow_off + crow_bytes;
        out.lds = out.need_off + need_bytes;
    }
    return true;
}

hipError_t launch_fused_rows_solve(const icnn_be_fc_model &m, const float *ctx, const icnn_be_state &st, float *f_work,
                                   float *g_work, int per_wg, long long *dual_prof, hipStream_t stream, bool resume,
                                   const SolveReset &reset, const RowsValue *value) {
    if (resume && reset.on) return hipErrorInvalidValue;
    if (value && (resume || st.variant != ICNN_BE_VARIANT_RL || !value->act)) return hipErrorInvalidValue;
    FusedRowsLayout lay;
    if (!fused_rows_layout(m, st, per_wg, resume, lay)) return hipErrorInvalidValue;
    FusedRowsArgs args{};
    int unused = 0;
    if (fill_args(m, args.fa, unused) != 0) return hipErrorInvalidValue;
    args.fa.ctx = ctx; args.fa.y = st.y; args.fa.f = f_work; args.fa.g = g_work; args.fa.finished = nullptr;
    args.fa.batch = st.batch; args.fa.prof = fc_profile_buffer();
    if (!make_dual_args(args.da, st, f_work, g_work, 0, 0, st.slots, dual_prof)) return hipErrorInvalidValue;
    rows_layout(m, per_wg, args.lay);
    args.sample_bytes = lay.sample_bytes;
    args.per_wg = per_wg;
    args.dual_off = lay.dual_off;
    args.crow_off = lay.crow_off;
    args.rounds = args.iters = st.iters > 0 ? st.iters : st.slots;
    args.resume = resume ? 1 : 0;
    args.reset = reset;
    if (value) args.value = *value;
    const bool big = st.slots > 15;
    const int which = (st.variant == ICNN_BE_VARIANT_RL ? 1 : 0) + (big ? 2 : 0);
    auto kern = which == 0 ? fused_rows_solve_kernel<false, 16> : which == 1 ? fused_rows_solve_kernel<true, 16>
              : which == 2 ? fused_rows_solve_kernel<false, 32> : fused_rows_solve_kernel<true, 32>;
    if (st.variant == ICNN_BE_VARIANT_PDIPM)
        kern = big ? fused_rows_solve_kernel<false, 32, 0, true> : fused_rows_solve_kernel<false, 16, 0, true>;
    if (!resume && dual_step_small_fits(st, 0))         // narrow rows, variant RL: all dual steps of the workgroup on wave 0
        kern = st.slots <= 5 ? fused_rows_solve_kernel<true, 16, 5> : st.slots <= 7 ? fused_rows_solve_kernel<true, 16, 8>
                                                                                  : fused_rows_solve_kernel<true, 16, 16>;
    if (value) {                                        // the same choice among the RL forms, with the value epilogue
        kern = big ? fused_rows_solve_kernel<true, 32, 0, false, true> : fused_rows_solve_kernel<true, 16, 0, false, true>;
        if (dual_step_small_fits(st, 0))
            kern = st.slots <= 5 ? fused_rows_solve_kernel<true, 16, 5, false, true>
                 : st.slots <= 7 ? fused_rows_solve_kernel<true, 16, 8, false, true> : fused_rows_solve_kernel<true, 16, 16, false, true>;
    }
    return launch_kernel(kern, dim3((st.batch + per_wg - 1) / per_wg), dim3(RTHREADS), lay.lds, stream, args);
}

namespace {
// The Bibsonomy network of the multi-label experiment (picnn.bibtex_spec(): 159 labels, hidden widths 600 and 159): the
// benchmark's model, whose shape does not change between the calls of a training or test run.
typedef FixedShape<159, 600, 159, 1> BibtexShape;

// Everything a fixed instance holds as a constant against what the launcher's own functions (fill_args with pack_offsets,
// make_dual_args with pw_build) produced for THIS model and state: the instance is taken only where all of it agrees.
template <typename Shape>
bool dual_shape_matches(const DualArgs &da) {       // the half a dual body holds: n, the row pitch, the pairwise-sum plan
    const PairwisePlan &p = da.plan, &q = Shape::PLAN;
    bool ok = da.st.n == Shape::N_ROW && da.n_pad == Shape::N_PAD && da.ldA == Shape::LDA &&
              p.n_leaves == q.n_leaves && p.n_prog == q.n_prog && p.depth == q.depth;
    for (int i = 0; ok && i < q.n_leaves; ++i) ok = p.leaf_start[i] == q.leaf_start[i] && p.leaf_len[i] == q.leaf_len[i];
    for (int i = 0; ok && i < q.n_prog; ++i) ok = p.prog[i] == q.prog[i];
    return ok;
}
template <typename Shape>
bool shape_matches(const FcArgs &fa, const DualArgs &da) {
    return fc_geom_same(fa, Shape::GEOM) && dual_shape_matches<Shape>(da);
}

// One round of a dual body that only the fixed instances above contain (icnn_be_debug_dual_step_body), on its own: one
// single-wave workgroup per sample, called the way fused_fc_solve_kernel calls it -- DualArgs first in the argument struct and
// handed on as a reference into the kernel-argument segment, the constant rows written once to LDS and shared, rows_cap formed
// as the ungrouped (rows_mode 0) or the grouped round loop (rows_mode 1: kk) forms it, the register budget of the 16-wave
// workgroup (the launch bound, not the launch, sets it).
struct BodyProbeArgs {
    DualArgs da;       // first: dual_step_body re-reads it at offset 0 of the kernel-argument segment
    int round, rounds, rows_mode, crow_off;
};
typedef const __attribute__((address_space(4))) BodyProbeArgs KPArgs;

template <int KT, int KCAP>
__global__ __launch_bounds__(NTHREADS) void dual_body_probe_kernel(BodyProbeArgs args) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    {
        float *crow = reinterpret_cast<float *>(smem + args.crow_off);  // behind the sample's region
        for (int j = thread_id(); j < 2 * BibtexShape::LDA; j += 64) crow[j] = j < BibtexShape::LDA ? 0.f : 1.f;
    }
    __syncthreads();
    KPArgs *kp = (KPArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    int u = blockIdx.x;
    asm volatile("" : "+s"(kp), "+s"(u));
    KPArgs &k = *kp;
    const int round = k.round;
    int rows_cap = round + 1 < k.da.st.slots ? round + 1 : k.da.st.slots;
    if (k.rows_mode) {                                              // the grouped loop: sized by the cuts the sample holds
        int kk = 0;
        if (k.da.st.finished[u] == 0 && k.da.st.t_next[u] < k.rounds) kk = k.da.st.count[u] + 1;
        kk = uni(kk);
        if (kk > k.da.st.slots) kk = k.da.st.slots;
        if (kk <= 0) return;
        rows_cap = kk;
    }
    using Body = DualCfgTile<DualCfg<float, KT, 1, false>, false, BibtexShape, KCAP>;     // as the tile kernel's instances
    dual_step_body<Body>(k.da, u, thread_id() & 63, smem, round, rows_cap, reinterpret_cast<const float *>(smem + k.crow_off));
}

// ICNN_BE_SHAPE_*: the instance a launch with these arguments and this layout takes
int pick_shape_instance(const FusedArgs &args, const FusedTileLayout &lay) {
    const icnn_be_state &st = args.da.st;
    if ((st.flags & ICNN_BE_FLAG_GENERIC_SHAPE) || st.variant != ICNN_BE_VARIANT_DUAL || st.cut_dtype != ICNN_BE_CUT_F32 ||
        args.da.budget > 0 || !shape_matches<BibtexShape>(args.fa, args.da))
        return ICNN_BE_SHAPE_GENERIC;
    const bool big = st.slots > 15;
    if (!big && !lay.grouped) return ICNN_BE_SHAPE_BIBTEX_KT16;
    if (big && lay.grouped) return ICNN_BE_SHAPE_BIBTEX_KT32_GROUPED;
    return ICNN_BE_SHAPE_GENERIC;
}

}  // namespace

int fused_shape_instance(const icnn_be_fc_model &m, const icnn_be_state &st, int tile_rows, int budget) {
    FusedArgs args{};       // what launch_fused_fc_solve fills, but for the buffers
    FusedTileLayout lay;
    int fg_bytes = 0;
    if (!fused_tile_layout(m, st, tile_rows, budget, lay) || fill_args(m, args.fa, fg_bytes) != 0 ||
        !make_dual_args(args.da, st, nullptr, nullptr, 0, budget, st.slots, nullptr))
        return ICNN_BE_SHAPE_GENERIC;
    return pick_shape_instance(args, lay);
}

hipError_t launch_fused_fc_solve(const icnn_be_fc_model &m, const float *ctx, const icnn_be_state &st, float *f_work,
                                 float *g_work, long long *dual_prof, hipStream_t stream, int tile_rows, int budget,
                                 const SolveReset &reset) {
    if (budget > 0 && reset.on) return hipErrorInvalidValue;
    FusedTileLayout lay;
    if (!fused_tile_layout(m, st, tile_rows, budget, lay)) return hipErrorInvalidValue;
    FusedArgs args{};
    int fg_bytes = 0;
    if (fill_args(m, args.fa, fg_bytes) != 0) return hipErrorInvalidValue;
    args.fa.ctx = ctx; args.fa.y = st.y; args.fa.f = f_work; args.fa.g = g_work; args.fa.finished = st.skip_fg;
    args.fa.batch = st.batch; args.fa.prof = fc_profile_buffer(); args.fa.tile_rows = tile_rows;   // (laps: profiling build only)
    if (!make_dual_args(args.da, st, f_work, g_work, 0, budget, st.slots, dual_prof)) return hipErrorInvalidValue;
    args.rounds = st.iters > 0 ? st.iters : st.slots;
    args.crow_off = lay.crow_off; args.samples_off = 0; args.sample_bytes = lay.sample_bytes;
    args.grouped = lay.grouped; args.group_cap = lay.group_cap; args.need_off = lay.need_off;
    args.trace = dual_trace_buffer();
    args.reset = reset;
    const bool rl = st.variant == ICNN_BE_VARIANT_RL, big = st.slots > 15;
    auto kern = big ? (rl ? fused_fc_solve_kernel<true, 32> : fused_fc_solve_kernel<false, 32>)
                    : (rl ? fused_fc_solve_kernel<true, 16> : fused_fc_solve_kernel<false, 16>);
    if (st.variant == ICNN_BE_VARIANT_PDIPM) kern = big ? fused_fc_solve_kernel<false, 32, true> : fused_fc_solve_kernel<false, 16, true>;
    if (budget > 0) kern = big ? fused_fc_solve_kernel<false, 32, false, true> : fused_fc_solve_kernel<false, 16, false, true>;
    switch (pick_shape_instance(args, lay)) {           // (never with a budget, never another variant)
    case ICNN_BE_SHAPE_BIBTEX_KT16:
        // the round classes are compiled for the fused VALU pass: a launch that keeps the MFMA sweep, or asks for the one body,
        // runs the instance without them
        kern = (st.flags & (ICNN_BE_FLAG_NO_ROUND_CLASSES | ICNN_BE_FLAG_MFMA_CONTRACTION))
                   ? fused_fc_solve_kernel<false, 16, false, false, BibtexShape, 0>
                   : fused_fc_solve_kernel<false, 16, false, false, BibtexShape, 0, true>;
        break;
    case ICNN_BE_SHAPE_BIBTEX_KT32_GROUPED: kern = fused_fc_solve_kernel<false, 32, false, false, BibtexShape, 1>; break;
    default: break;
    }
    return launch_kernel(kern, dim3((st.batch + tile_rows - 1) / tile_rows), dim3(NTHREADS), lay.lds, stream, args);
}

hipError_t launch_dual_body_probe(const icnn_be_state &st, int round, const void *f, const void *g, int which, int rows_mode,
                                  hipStream_t stream) {
    BodyProbeArgs args{};
    if (st.variant != ICNN_BE_VARIANT_DUAL || st.cut_dtype != ICNN_BE_CUT_F32 ||
        (st.flags & (ICNN_BE_FLAG_GLOBAL_BUNDLE | ICNN_BE_FLAG_TIME_SLICE)) ||
        !make_dual_args(args.da, st, f, g, round, 0, st.slots, nullptr) || !dual_shape_matches<BibtexShape>(args.da))
        return hipErrorInvalidValue;
    const bool big = st.slots > 15;
    if (which < 1 || which > 3 || big != (which == 3) || rows_mode < 0 || rows_mode > 1 || (rows_mode == 1 && which == 2))
        return hipErrorInvalidValue;
    // the capped body is compiled for rows_cap <= round + 1 <= its cap and for the fused VALU pass
    if (which == 2 && (round >= ROUND_CLASS_CAP || (st.flags & ICNN_BE_FLAG_MFMA_CONTRACTION))) return hipErrorInvalidValue;
    if (st.batch == 0) return hipSuccess;
    args.round = round;
    args.rounds = st.iters > 0 ? st.iters : st.slots;
    args.rows_mode = rows_mode;
    args.crow_off = sample_region_bytes(st, args.da.ldA, args.da.n_pad, args.da.plan.n_leaves);
    const int lds = args.crow_off + ((2 * args.da.ldA * 4 + 15) & ~15);
    auto kern = which == 1 ? dual_body_probe_kernel<16, 0> : which == 2 ? dual_body_probe_kernel<16, ROUND_CLASS_CAP>
                                                                        : dual_body_probe_kernel<32, 0>;
    return launch_kernel(kern, dim3(st.batch), dim3(64), lds, stream, args);
}

}  // namespace icnn_be
