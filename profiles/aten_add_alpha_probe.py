#!/usr/bin/env python3
"""Does ATen's add(alpha=) on this GPU round `a + alpha * b` once (a fused multiply-add) or twice (multiply, then add)?

    python profiles/aten_add_alpha_probe.py [--out FILE]

The optimizers' weight-decay, dampened-momentum and Nesterov terms are such adds, and
csrc/optim.hip must round them as ATen does.  For 4 M random float32 pairs and four alphas this counts the elements where
torch.add / Tensor.add_ on the device differ bitwise from each host-side form:
  fused:    float32(a + alpha32 * b) evaluated in float64 (the product of two float32 is exact there)
  separate: float32(float32(alpha32 * b) + a)
Prints one JSON line (and writes it to --out).
"""
import argparse
import json

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aten_add_alpha_probe.py needs a GPU")
    torch.manual_seed(0)
    n = 1 << 22
    a = torch.randn(n, device="cuda")
    b = torch.randn(n, device="cuda")
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    rows = []
    for alpha in (0.3, 5e-4, 0.9, 1e-4):
        a32 = np.float32(alpha)
        fused = (an.astype(np.float64) + bn.astype(np.float64) * np.float64(a32)).astype(np.float32).view(np.uint32)
        sep = (an + bn * a32).astype(np.float32).view(np.uint32)
        for op, r in (("add", torch.add(a, b, alpha=alpha)), ("add_", a.clone().add_(b, alpha=alpha))):
            r = r.cpu().numpy().view(np.uint32)
            rows.append({"alpha": alpha, "op": op, "mismatch_vs_fused": int((r != fused).sum()),
                         "mismatch_vs_separate": int((r != sep).sum())})
    line = json.dumps({"probe": "aten_add_alpha", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                       "pairs": n, "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
