#!/usr/bin/env python3
"""Spot checks of the reference recorded as data, for the CPU tests that once imported the reference live:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_spot_golden.py <path of the reference checkout>

  shim_golden.json             the reference's CIFAR MobileNetV1_Q and ImageNet SqueezeNet, built and run by the
                               reference on its OWN utils: MobileNetV1_Q(ch_in=3, qbit=32) with netgen.fill_parameters
                               (the same state-dict values on both sides) and its logits for netgen.net_input(batch=2)
                               (q_bit 32 = the passthrough, so a CPU forward is defined), the number of Conv2d modules of
                               MobileNetV1_Q(qbit=8) and of SqueezeNet(qbit=7).
  quantizer_spot_golden.json   the reference's quantize_act / quantize_weight for Qbits 8 and 7 on 2^18 seeded
                               N(0, 5^2) float32 inputs: SHA-256 digests of the inputs' and of every output's bits.

tests/test_abi_host.py rebuilds the nets out of THIS repo's drop-in modules (tests/golden/netgen.py,
tests/golden/netgen_r3.py); tests/test_oracle_golden.py runs the oracle on the same inputs.  Only data is stored."""
import hashlib
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

QUANT_SEED, QUANT_N, QUANT_SCALE = 20240, 1 << 18, 5.0
SHIM_PARAM_SEED, SHIM_INPUT_SEED, SHIM_BATCH = 2024, 99, 2


def quantizer_inputs(torch):
    """The inputs of quantizer_spot_golden.json (also drawn by the test)."""
    g = torch.Generator().manual_seed(QUANT_SEED)
    return torch.randn(QUANT_N, generator=g) * QUANT_SCALE


def bits_sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype("<u4").tobytes()).hexdigest()


def dump(name, obj):
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


def main(ref):
    warnings.filterwarnings("ignore")
    sys.path.insert(0, ref)
    sys.modules["torchsummary"] = types.ModuleType("torchsummary")
    sys.modules["torchsummary"].summary = lambda *a, **k: None
    import torch
    import utils.conv2d_func as ref_cf
    from utils.sfp_quant import quantize_act, quantize_weight
    from nets_cifar.mobilenetv1 import MobileNetV1_Q
    from nets_imgnet.squeezenet1_0 import SqueezeNet
    assert os.path.abspath(ref_cf.__file__).startswith(os.path.abspath(ref)), "must import the REFERENCE utils"

    sys.path.append(HERE)
    import netgen
    m = netgen.fill_parameters(MobileNetV1_Q(ch_in=3, qbit=32), seed=SHIM_PARAM_SEED).eval()
    with torch.no_grad():
        y = m(netgen.net_input(batch=SHIM_BATCH, seed=SHIM_INPUT_SEED))
    n_conv = lambda net: sum(1 for mod in net.modules() if isinstance(mod, torch.nn.Conv2d))  # noqa: E731
    dump("shim_golden.json", {"mobilenetv1_cifar_q32": {"param_seed": SHIM_PARAM_SEED, "input_seed": SHIM_INPUT_SEED,
                                                        "batch": SHIM_BATCH,
                                                        "logits": [float(v) for v in y.flatten()],
                                                        "logits_shape": list(y.shape),
                                                        "abs_sum": float(y.double().abs().sum())},
                              "mobilenetv1_cifar_q8_n_conv": n_conv(MobileNetV1_Q(ch_in=3, qbit=8)),
                              "squeezenet_q7_n_conv": n_conv(SqueezeNet(qbit=7))})

    x = quantizer_inputs(torch)
    out = {"seed": QUANT_SEED, "n": QUANT_N, "scale": QUANT_SCALE, "input_sha256": bits_sha256(x.numpy())}
    for b in (8, 7):
        out[f"act{b}_sha256"] = bits_sha256(quantize_act(b)(x).numpy())
        out[f"w{b}_sha256"] = bits_sha256(quantize_weight(b)(x).numpy())
    dump("quantizer_spot_golden.json", out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
