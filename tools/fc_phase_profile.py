#!/usr/bin/env python3
"""Per-phase cycle breakdown of fc_fg_kernel on the benchmark workload (GPU box only): diagnostic hook
icnn_be_debug_profile_fc, s_memtime laps by lane 0 of every wave of every workgroup.
    fc_phase_profile.py [B [bibtex|rl [adam [iters]]]]     one icnn_be_fc_fg launch (or the persistent Adam loop)
    fc_phase_profile.py B --fused [nIter]                  the evaluations inside one fused_fc_solve_kernel launch, per round"""
import ctypes as C
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from icnn_amd import _lib, picnn  # noqa: E402

_lib.use_profiling_build()            # the laps are compiled into the profiling variant of the library only

PH = ["input: y, y*yu_i operands", "-", "L0 tiles + epilogue", "L0 barrier wait", "-", "L1 tiles + epilogue", "L1 barrier wait",
      "E rows", "bwd1 delta0 (+ dE/dy_1 where it stays)", "bwd1 barrier wait", "bwd0 dE/dy_0 chain", "bwd0 dE/dy_1 units",
      "bwd0 barrier wait", "g epilogue + store", "adam: entropy, best, stop rule", "adam: moments, step"]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
if len(sys.argv) > 2 and sys.argv[2] == "rl":          # the RL agent's 200-200 negQ network (same phase list)
    spec = picnn.halfcheetah_spec()
    params = picnn.init_params(spec, 0, "spread", yu_bias=1.0, gate_bias=1.0)
    x = torch.from_numpy(np.random.RandomState(1000).randn(max(B, 64), spec.n_features).astype(np.float32)).cuda()
else:
    spec = picnn.bibtex_spec()
    params = picnn.init_params(spec, 0, "spread")
    x = torch.from_numpy((np.random.RandomState(1000).rand(B, spec.n_features) < 0.04).astype(np.float32)).cuda()
model = picnn.FCModel(spec, params)
ctx = model.context(x)[:B].contiguous()
y = torch.full((B, spec.n_labels), 0.5, dtype=torch.float64, device="cuda")
FUSED = len(sys.argv) > 2 and sys.argv[2] == "--fused"    # the evaluations inside the persistent tile solve, per round
ADAM = len(sys.argv) > 3 and sys.argv[3] == "adam"      # profile the persistent Adam loop instead (per iteration)
if ADAM:
    import dataclasses

    from icnn_amd import rl_adam
    model = picnn.FCModel(dataclasses.replace(spec, action_box=False), params)
    solver = rl_adam.AdamSolver(model, B, int(sys.argv[4]) if len(sys.argv) > 4 else 1000)
    solver.solve(ctx)
if FUSED:
    from icnn_amd import bundle_entropy
    n_iter = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    fs = bundle_entropy.FusedSolver(model, B, n_iter, "dual")
    fs.solve(ctx, 0.5)
for _ in range(3):
    model.fg(ctx, y)
torch.cuda.synchronize()
nwg = B if FUSED else (B + 15) // 16       # (fused: 4- and 8-row tiles at small batches)
prof = torch.zeros(nwg, 16, 16, dtype=torch.int64, device="cuda")
lib = _lib.load()
lib.icnn_be_debug_profile_fc(C.c_void_p(prof.data_ptr()))
if ADAM:
    evals = int(solver.solve(ctx).iters.item()) + 1
elif FUSED:
    fs.solve(ctx, 0.5)
    evals = n_iter
else:
    model.fg(ctx, y)
    evals = 1
torch.cuda.synchronize()
lib.icnn_be_debug_profile_fc(None)
p = prof.cpu().numpy().astype(np.float64) / evals
p = p[p.sum((1, 2)) > 0]
if ADAM:
    print("Adam loop: %d PICNN evaluations; cycles below are per evaluation" % evals)
tot = p.sum(2)
if FUSED:
    print("fused solve, %d rounds: cycles below are per round (samples that finish early leave their tile's later rounds empty)" % evals)
print("cycles per wave for one fc_fg launch: mean %.0f  max %.0f  (%.1f us at 2.4 GHz)" % (tot.mean(), tot.max(), tot.mean() / 2400))
for i, name in enumerate(PH[:16 if ADAM else 14]):
    print("  %-30s mean %8.0f (%5.1f%%)   wave-min %8.0f  wave-max %8.0f" %
          (name, p[:, :, i].mean(), 100 * p[:, :, i].sum() / tot.sum(), p[:, :, i].mean(0).min(), p[:, :, i].mean(0).max()))
