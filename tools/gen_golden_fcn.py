#!/usr/bin/env python3
"""Writes tests/golden/fcn_baseline__k16_16x24.npz from the reference's own completion/baseline.py (CPU only):
    python tools/gen_golden_fcn.py --reference /path/to/the/reference/tree
The script itself cannot be imported (it needs setproctitle, IPython and the olivetti module at import time), so the FCN class
definition, the expression its loop assigns to `loss` (baseline.py:94) and the one that makes its optimiser (baseline.py:78)
are taken out of its syntax tree and evaluated with torch, nn, F and optim in scope.  Three steps of forward, that loss,
zero_grad, backward, step run on B = 3 seeded uniform images of 16 x 24 with uniform targets.  The file holds data only: theta_0 as named arrays (theta0/<name>), x, t [3, 16, 24], yhat of the
first forward, the three losses, the flat gradients of the three steps (grad1..3: the update is pinned from the reference's own
gradients) and the flat theta after step 3, all float32."""
import argparse
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn, optim

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, B, H, W, STEPS = 16, 3, 16, 24, 3


def reference_pieces(tree_root):
    """(the FCN class, the loss expression, the optimiser expression) of the reference's script, as compiled syntax trees"""
    path = os.path.join(tree_root, "completion", "baseline.py")
    tree = ast.parse(open(path).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FCN"]
    if not cls:
        raise SystemExit("no class FCN in %s" % path)
    scope = {"nn": nn, "F": F, "torch": torch}
    exec(compile(ast.Module(body=cls, type_ignores=[]), path, "exec"), scope)

    def assigned(name):
        for n in ast.walk(tree):
            if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name) and n.targets[0].id == name:
                return compile(ast.Expression(body=n.value), path, "eval")
        raise SystemExit("no assignment to %s in %s" % (name, path))

    return scope["FCN"], assigned("loss"), assigned("opt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds completion/baseline.py)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "fcn_baseline__k16_16x24.npz"))
    args = ap.parse_args()
    torch.manual_seed(0)
    FCN, loss_expr, opt_expr = reference_pieces(args.reference)
    model = FCN(k=K)
    rng = np.random.RandomState(0)
    x = rng.uniform(0.0, 1.0, (B, H, W)).astype(np.float32)
    t = rng.uniform(0.0, 1.0, (B, H, W)).astype(np.float32)
    out = {"theta0/" + name: p.detach().numpy().copy() for name, p in model.named_parameters()}
    xt, tt = torch.from_numpy(x).view(B, 1, H, W), torch.from_numpy(t).view(B, 1, H, W)
    opt = eval(opt_expr, {"optim": optim, "model": model})
    assert isinstance(opt, optim.Adam) and opt.defaults["lr"] == 1e-4
    losses = []
    for step in range(STEPS):
        yhat = model(xt)
        loss = eval(loss_expr, {"yhat": yhat, "y": tt})
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        if step == 0:
            out["yhat"] = yhat.detach().numpy().reshape(B, H, W).copy()
        out["grad%d" % (step + 1)] = np.concatenate([p.grad.numpy().reshape(-1) for p in model.parameters()])
        opt.step()
    out.update(x=x, t=t, losses=np.asarray(losses, np.float32),
               theta3=np.concatenate([p.detach().numpy().reshape(-1) for p in model.parameters()]))
    np.savez(args.out, **out)
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)), file=sys.stderr)


if __name__ == "__main__":
    main()
