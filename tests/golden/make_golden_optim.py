#!/usr/bin/env python3
"""Generate tests/golden/optim_golden.npz from the IMPORTED reference optimizers (utils/optimizer.py), on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_optim.py --reference DIR

DIR is a checkout of the reference (the directory holding its `utils/`).  Its optimizer module imports torchvision
without using it; a stub stands in for it here.  The fixture holds the reference's own outputs over three steps --
p, p.grad and state['momentum_buffer'] after every step -- for DSGD and SSGD with qbit 8, 7 and 32 and for NormalSGD,
each with momentum 0 and 0.9.  weight_decay = 0 and dampening = 0, so every `a + alpha * b` of the step has alpha 1
and the CPU and GPU results cannot differ by a contracted multiply-add.

Layout: p0 (initial weights), g1..g3 (the gradient assigned before each step), grad_s{k} (p.grad after step k, the
same for every case: the generator checks that), and per case `{rule}_q{qbit}_m{0|9}`:  <case>_p_s{k} and, with
momentum, <case>_buf_s{k}.  NormalSGD is stored as qbit 32 (it has no quantizer).
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_STEPS = 3
LR = 0.01
QBITS = (8, 7, 32)
MOMENTA = (0.0, 0.9)


def f32(x):
    return np.asarray(x, dtype=np.float32)


def edges():
    """Quantizer bin edges and class boundaries of SLFP<3,4> weights and SFP<3,3>, and the float32 neighbours of each."""
    out = [0.0625, 0.125, 15.0, 15.32165, 1e-10]
    for e in (-4, -2, 0, 1, 3):
        out += [2.0 ** (e + (k + 0.5) / 16) for k in range(16)]   # log-domain rounding midpoints (weights, 8 bit)
        out += [2.0 ** e * (1 + (j + 0.5) / 8) for j in range(8)]  # linear rounding midpoints (7 bit)
    v = f32(out)
    near = [v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(0)),
            np.nextafter(np.nextafter(v, f32(np.inf)), f32(np.inf))]
    return np.concatenate(near)


def make_inputs(n, rng):
    special = f32([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e-38, -1e-38, 1e-10, -1e-10, 1e-4, -1e-4,
                   0.06249, 0.0625, -0.0625, 0.12499, 0.125, -0.125, 15.32, 15.33, -15.33, 100.0, -1e30])
    e = edges()
    e = np.concatenate([e, -e[: len(e) // 2]])
    body = rng.standard_normal(n).astype(np.float32) * f32(0.5)
    p0 = np.concatenate([special, e, body])[:n].astype(np.float32)
    gs = []
    for k in range(N_STEPS):
        g = (rng.standard_normal(n) * 0.01).astype(np.float32)
        # |lr * g| around 1e-4: the qbit-32 DSGD mask straddles its threshold
        idx = rng.choice(n, n // 8, replace=False)
        g[idx] = f32(1e-2) * (1 + rng.integers(-3, 4, idx.size).astype(np.float32) * f32(2.0 ** -20))
        # steps large enough to cross bins
        idx = rng.choice(n, n // 16, replace=False)
        g[idx] = (rng.standard_normal(idx.size) * 3).astype(np.float32)
        g[:8] = f32([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, np.nan])
        g[8 + 3 * k] = f32(np.inf)  # non-finite entries that move from step to step
        g[40 + 5 * k] = f32(np.nan)
        gs.append(g)
    return p0, gs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="reference checkout (the directory holding utils/)")
    ap.add_argument("-n", type=int, default=1024)
    args = ap.parse_args()
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))  # imported, never used
    sys.path.insert(0, os.path.abspath(args.reference))
    import torch
    from utils import optimizer as ref  # the REFERENCE module
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(args.reference)), ref.__file__

    rng = np.random.default_rng(20261016)
    p0, gs = make_inputs(args.n, rng)
    out = {"p0": p0, "lr": f32(LR)}
    for k, g in enumerate(gs, 1):
        out[f"g{k}"] = g
    cases = [(r, q, m) for r in ("DSGD", "SSGD") for q in QBITS for m in MOMENTA] + [("NormalSGD", 32, m) for m in MOMENTA]
    for rule, q, m in cases:
        p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        if rule == "NormalSGD":
            opt = ref.NormalSGD([p], lr=LR, momentum=m)
        else:
            opt = getattr(ref, rule)([p], qbit=q, lr=LR, momentum=m)
        name = f"{rule}_q{q}_m{int(m * 10)}"
        for k, g in enumerate(gs, 1):
            p.grad = torch.from_numpy(g.copy())
            opt.step()
            out[f"{name}_p_s{k}"] = p.detach().numpy().copy()
            grad = p.grad.numpy().copy()
            key = f"grad_s{k}"
            if key in out:
                assert out[key].view(np.uint32).tobytes() == grad.view(np.uint32).tobytes(), (name, k)
            out[key] = grad
            if m:
                out[f"{name}_buf_s{k}"] = opt.state[p]["momentum_buffer"].numpy().copy()
    path = os.path.join(HERE, "optim_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
