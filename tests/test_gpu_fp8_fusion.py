"""GPU (MI355X): fusion.use_fp8_operands on the small Fire-module net of tests/test_gpu_fire.py at q_bit 7."""
import pytest
import torch

from test_gpu_fire import _small_fire_net

pytestmark = pytest.mark.gpu


def _linked():
    from cnns_slfp_quantization_amd import fusion
    assert torch.cuda.is_available(), "this test needs the MI355X"
    m, x = _small_fire_net(torch.device("cuda:0"))
    with torch.no_grad():
        assert fusion.fuse_fire(m, x) == 1
    return fusion, m, x, [m.fire.squeeze, m.fire.expand1x1, m.head]   # the 1x1 layers fuse_fire links; expand3x3 stays on the dense kernel


def test_use_fp8_operands_marks_the_linked_1x1_layers_and_restores():
    fusion, m, x, ones = _linked()
    keys = sorted(m.state_dict())
    with torch.no_grad():
        y0 = m(x)
        assert fusion.use_fp8_operands(m, x, rtol=1e-5) == len(ones)
        y1 = m(x)
        assert all(c._fp8 and c._last_kernel.startswith("pw_mfma_fp8+codes_in") for c in ones) and not m.fire.expand3x3._fp8
        assert "+slice" in m.fire.expand1x1._last_kernel and sorted(m.state_dict()) == keys
        err = float((y1 - y0).abs().max() / y0.abs().max())
        print("logits moved by", err)
        assert err <= 1e-5
        assert fusion.restore_fp8_operands(m) == len(ones)
        assert torch.equal(m(x), y0) and not m.head._last_kernel.startswith("pw_mfma_fp8")


def test_rtol_zero_refuses_a_model_whose_output_moves():
    fusion, m, x, ones = _linked()
    with torch.no_grad():
        y0 = m(x)
        assert fusion.use_fp8_operands(m, x, rtol=None) == len(ones)
        moved = not torch.equal(m(x), y0)
        assert fusion.restore_fp8_operands(m) == len(ones)
        if not moved:
            pytest.skip("the E4M3 kernels are bit-equal to the fp16 kernels on this net: rtol=0.0 has nothing to refuse")
        with pytest.raises(RuntimeError, match="nothing was changed"):
            fusion.use_fp8_operands(m, x, rtol=0.0)
        assert not any(c._fp8 for c in ones)
