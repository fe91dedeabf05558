"""CPU: the host logic that fusion.py's passes share -- the forward trace, the tensor-identity rule, the
wrap / unwrap records and the verify-or-roll-back helper -- on a hand-wired block of q_bit 32 Conv2d_Q modules, which run stock
ATen on the CPU with their forward hooks firing.  No device work is done here."""
import weakref

import pytest
import torch
import torch.nn as nn

from cnns_slfp_quantization_amd import _lib, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf

STATE = ("_post", "_code_out", "_code_entry", "_trunk_code_out", "residual_relu")
MARKERS = ("_in_residual", "_pre_link_post", "_stem_link", "_trunk_link", "_fire_fused", "_residual_fused", "_named_bn",
           "_fused_modules", "_dw_slot", "forward")


class _Join(nn.Module):
    def forward(self, a, b):
        return a + b


class _Block(nn.Module):
    """conv -> nn.Identity -> in-place ReLU -> MaxPool2d -> two convs that read the pooled tensor, each followed by the same
    (not in-place) ReLU module -> a module with two inputs: nine leaf calls."""

    def __init__(self, fail=False):
        super().__init__()
        C = cf.conv2d_Q(q_bit=32, Kw=0.02, Ka=0.25)
        self.conv = C(3, 8, 3, 0.02, 0.25, 1, 1)
        self.idt = nn.Identity()
        self.relu = nn.ReLU(inplace=True)
        self.pool = nn.MaxPool2d(3, 2, 1)
        self.a = C(8, 8, 1, 0.02, 0.3)
        self.b = C(8, 8, 3, 0.02, 0.3, 1, 1)
        self.act = nn.ReLU()
        self.join = _Join()
        self.fail = fail

    def forward(self, x):
        p = self.pool(self.relu(self.idt(self.conv(x))))
        if self.fail:
            raise ValueError("a forward that raises after some hooks have fired")
        return self.join(self.act(self.a(p)), self.act(self.b(p)))


def _model(fail=False):
    torch.manual_seed(3)
    m = _Block(fail).eval()
    return m, torch.randn(2, 3, 9, 11, generator=torch.Generator().manual_seed(4))


def _hooks(m):
    return sum(len(c._forward_hooks) + len(c._forward_pre_hooks) for c in m.modules())


def _state(m):
    return ([(name, id(mod)) for name, mod in m.named_modules()],
            [tuple(id(c.__dict__[k]) if k == "_post" else c.__dict__[k] for k in STATE) for c in m.modules() if fusion._is_conv_q(c)],
            [tuple(k in c.__dict__ for k in MARKERS) for c in m.modules()])


# ---------------------------------------------------------------------------------------------- the trace
def test_trace_records_the_calls_in_execution_order_and_follows_tensors():
    m, x = _model()
    tr = fusion._Trace(m, x)
    assert [c.mod for c in tr.calls] == [m.conv, m.idt, m.relu, m.pool, m.a, m.act, m.b, m.act, m.join]
    assert all(isinstance(c.inp, tuple) for c in tr.calls) and tr.calls[0].x is x and tr.calls[-1].out is tr.output
    conv, idt, relu, pool = tr.calls[:4]
    # nn.Identity and the in-place ReLU hand on the conv's tensor; the pool makes another one
    assert tr.same(conv.out, idt.out) and tr.same(conv.out, relu.out) and tr.same(relu.out, pool.x)
    assert not tr.same(pool.x, pool.out) and not tr.same(conv.out, x)
    assert not tr.same(pool.out, None) and not tr.same(None, pool.out) and tr.same(None, None)
    # the same address, shape, dtype and strides without being the same object -- and not with other strides or another shape
    assert tr.same(pool.out, pool.out.view(pool.out.shape)) and not tr.same(pool.out, pool.out.flatten())
    assert not tr.same(pool.out, pool.out.permute(0, 1, 3, 2)) and not tr.same(pool.out, pool.out[:, :, :, :1])
    assert [tr.runs(mod) for mod in (m.conv, m.act, m.join, m)] == [1, 2, 1, 0]   # the container is not recorded
    assert [c.mod for c in tr.of(m.act)] == [m.act, m.act] and tr.of(m) == []


def test_io_is_none_unless_a_module_ran_once_with_one_tensor_in_and_out():
    m, x = _model()
    tr = fusion._Trace(m, x, blocks=[m])
    assert tr.calls[-1].mod is m and tr.runs(m) == 1   # a block is recorded although it is no leaf, after its children
    xin, out = tr.io(m)
    assert xin is x and out is tr.output
    assert tr.io(m.pool)[0] is tr.calls[3].x and tr.io(m.pool)[1] is tr.calls[3].out
    assert tr.io(m.act) is None     # ran twice
    assert tr.io(m.join) is None    # two positional inputs
    assert tr.io(nn.ReLU()) is None   # never ran


def test_readers_and_producer_of_a_tensor_with_two_consumers():
    m, x = _model()
    tr = fusion._Trace(m, x)
    pooled, conv_out = tr.io(m.pool)[1], tr.io(m.conv)[1]
    assert [c.mod for c in tr.readers(pooled)] == [m.a, m.b]
    assert [c.mod for c in tr.readers(conv_out)] == [m.idt, m.relu, m.pool]   # one tensor through nn.Identity and the in-place ReLU
    assert tr.readers(tr.output) == [] and tr.readers(None) == []
    assert tr.producer(pooled, lambda mod: True).mod is m.pool
    assert tr.producer(pooled, fusion._is_conv_q) is None and tr.producer(None, lambda mod: True) is None
    # three calls returned the conv's tensor: the kind says which one is meant
    assert tr.producer(conv_out, fusion._is_conv_q).mod is m.conv
    assert tr.producer(conv_out, lambda mod: isinstance(mod, nn.ReLU)).mod is m.relu
    assert tr.producer(tr.io(m.a)[1], fusion._is_conv_q).mod is m.a


def test_no_hook_outlives_a_trace_even_when_the_forward_raises():
    m, x = _model()
    fusion._Trace(m, x)
    assert _hooks(m) == 0
    m, x = _model(fail=True)
    with pytest.raises(ValueError, match="after some hooks have fired"):
        fusion._Trace(m, x)
    assert _hooks(m) == 0


def test_release_lets_go_of_the_recorded_tensors():
    m, x = _model()
    tr = fusion._Trace(m, x)
    pooled = weakref.ref(tr.io(m.pool)[1])   # (not a conv's output: the module keeps that in `.output`)
    y = tr.output
    assert pooled() is not None
    tr.release()
    assert pooled() is None
    assert tr.calls == [] and tr.runs(m.pool) == 0 and tr.io(m.pool) is None and tr.output is y


# ---------------------------------------------------------------------------------------------- the small helpers
def test_wrap_and_unwrap_are_inverse():
    m, x = _model()
    named = list(m.named_modules())
    orig = dict(named)
    recs = fusion._wrap_children(m, [m.pool], 7, relus=[m.relu, m.act])
    assert sorted(r[1] for r in recs) == ["act", "pool", "relu"] and all(r[0] is m for r in recs)
    assert isinstance(m.pool, fusion.CodeMaxPool2d) and m.pool.q_bit == 7 and m.pool.pool is orig["pool"]
    assert isinstance(m.relu, fusion.CodeReLU) and isinstance(m.act, fusion.CodeReLU) and m.relu.relu is orig["relu"]
    assert fusion._wrap_children(m, [orig["pool"]], 7) == []   # a wrapped pool is not wrapped again
    assert torch.equal(m(x), _model()[0](x))                 # float32 goes to the original modules
    m.act = nn.Identity()                                     # a slot that holds something else by now is left alone
    fusion._unwrap_children(recs)
    assert isinstance(m.act, nn.Identity)
    m.act = orig["act"]
    assert [(n, id(c)) for n, c in m.named_modules()] == [(n, id(c)) for n, c in named]
    assert fusion._wrap_children(m, [], 8) == []


def test_predicates_and_flag_helpers():
    C8 = cf.conv2d_Q_bias(q_bit=8, Kw=0.02, Ka=0.25)
    c = C8(8, 8, 1, 0.02, 0.25).eval()
    assert fusion._post_flags(c) == 0 and fusion._reader_quant(c) == (0.25, 8)
    assert fusion._code_eligible(c) and fusion._code_eligible(c, producer_side=True)
    fusion._fold_flags(c, 1)
    assert c._post == (None, None, 1) and fusion._post_flags(c) == 1 and fusion._code_eligible(c)
    scale = torch.ones(8)
    c._post = (scale, scale, 2)
    assert not fusion._code_eligible(c)                 # the layer-output quantizer
    fusion._fold_flags(c, 1)
    assert c._post[0] is scale and c._post[1] is scale and c._post[2] == 1
    c._code_out = (0.3, 8)
    assert fusion._code_eligible(c) and not fusion._code_eligible(c, producer_side=True)   # already writes codes
    c._code_out = None
    c._in_residual = True
    assert fusion._code_eligible(c) and not fusion._code_eligible(c, producer_side=True)   # its output is a block's trunk
    del c._in_residual
    assert not fusion._code_eligible(c.train()) and fusion._code_eligible(c.eval())
    assert not fusion._code_eligible(cf.conv2d_Q(8, 0.02, 0.25)(8, 8, 1, 0.02, 0.25, bias=True).eval())   # a raw bias
    assert not fusion._code_eligible(cf.conv2d_Q(32, 0.02, 0.25)(8, 8, 1, 0.02, 0.25).eval())
    assert not fusion._code_eligible(C8(8, 8, 3, 0.02, 0.25, 1, "same").eval())
    assert not fusion._code_eligible(nn.Conv2d(8, 8, 1).eval())


# ---------------------------------------------------------------------------------------------- the verifier
def _undo_counter():
    calls = []
    return calls, lambda: calls.append(1)


def test_verified_accepts_only_a_bit_equal_tensor():
    want = torch.arange(12, dtype=torch.float32).view(3, 4)
    calls, undo = _undo_counter()
    assert fusion._verified(lambda: want.clone(), want, undo) is True and calls == []
    assert fusion._verified(lambda: want.clone(), lambda: want, undo) is True and calls == []   # `want` made after fn has run
    off = want.clone()
    off[2, 3] += 1

    def raises():
        raise RuntimeError("an op that cannot take codes")

    refusals = [("dtype", lambda: want.double()), ("shape", lambda: want.view(4, 3)), ("one element", lambda: off),
                ("no tensor", lambda: (want,)), ("None", lambda: None), ("RuntimeError", raises)]
    for i, (name, fn) in enumerate(refusals):
        assert fusion._verified(fn, want, undo) is False, name
        assert len(calls) == i + 1, name   # undo ran exactly once per refusal
    assert torch.is_grad_enabled() and fusion._verified(lambda: torch.tensor([float(torch.is_grad_enabled())]), torch.zeros(1), undo)


def test_verified_warns_only_about_an_exception_and_names_it():
    calls, undo = _undo_counter()
    with pytest.warns(UserWarning, match=r"^pass: block raised KeyError: 'k'; restored$"):
        assert fusion._verified(lambda: {}["k"], torch.zeros(1), undo, warn="pass: block raised {}; restored") is False
    assert calls == [1]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert fusion._verified(lambda: torch.ones(1), torch.zeros(1), undo, warn="pass: {}") is False   # a mismatch: no warning
    assert calls == [1, 1]


def test_verified_reraises_a_library_error_after_the_roll_back_only_where_asked():
    def defect():
        raise _lib.SlfpError(_lib.ERR_UNSUPPORTED, "slfp_conv2d_fwd_codes: a call the support query had granted failed")

    calls, undo = _undo_counter()
    with pytest.raises(_lib.SlfpError, match="had granted"):
        fusion._verified(defect, torch.zeros(1), undo, reraise=True)
    assert calls == [1]
    assert fusion._verified(defect, torch.zeros(1), undo) is False   # link_codes_traced, fuse_residual: a refusal
    assert calls == [1, 1]


# ---------------------------------------------------------------------------------------------- the public passes on a CPU model
PASSES = [
    ("link_codes", lambda m, x: fusion.link_codes(m, example_input=x)),
    ("link_codes_traced", lambda m, x: fusion.link_codes_traced(m, x)),
    ("link_codes_traced entries", lambda m, x: fusion.link_codes_traced(m, x, entries=True)),
    ("link_stem", lambda m, x: fusion.link_stem(m, x)),
    ("fuse_residual", lambda m, x: fusion.fuse_residual(m, x)),
    ("link_trunk", lambda m, x: fusion.link_trunk(m, x)),
    ("fuse_fire", lambda m, x: fusion.fuse_fire(m, x)),
    ("fuse_fire entries", lambda m, x: fusion.fuse_fire(m, x, entries=True)),
    ("unlink_codes", lambda m, x: fusion.unlink_codes(m)),
    ("unlink_stem", lambda m, x: fusion.unlink_stem(m)),
    ("unfuse_residual", lambda m, x: fusion.unfuse_residual(m)),
    ("unlink_trunk", lambda m, x: fusion.unlink_trunk(m)),
    ("unfuse_fire", lambda m, x: fusion.unfuse_fire(m)),
    ("unfuse_named_bn", lambda m, x: fusion.unfuse_named_bn(m)),
    ("unfuse_dw_pw", lambda m, x: fusion.unfuse_dw_pw(m)),
    ("unfuse", lambda m, x: fusion.unfuse(m)),
]


@pytest.mark.parametrize("name, call", PASSES, ids=[p[0] for p in PASSES])
def test_every_pass_and_undo_leaves_a_cpu_model_alone(name, call):
    m, x = _model()
    before = _state(m)
    assert call(m, x) == 0
    assert _state(m) == before
    assert _hooks(m) == 0


# ---------------------------------------------------------------------------------------------- a pass that rewrites on the CPU
class _Bottleneck(nn.Module):
    """The torchvision child names on q_bit 32 modules: fuse_residual's candidate test does not ask for a kernel, and
    conv3(h, residual=identity) computes the add and the ReLU with ATen."""

    def __init__(self, gain=1.0):
        super().__init__()
        C = cf.conv2d_Q(q_bit=32, Kw=0.02, Ka=0.25)
        self.conv1, self.bn1 = C(8, 4, 1, 0.02, 0.25), nn.Identity()
        self.conv2, self.bn2 = C(4, 4, 3, 0.02, 0.25, 1, 1), nn.Identity()
        self.conv3, self.bn3 = C(4, 8, 1, 0.02, 0.25), nn.Identity()
        self.relu = nn.ReLU()
        self.downsample = None
        self.gain = gain

    def forward(self, x):
        h = self.relu(self.bn1(self.conv1(x)))
        h = self.relu(self.bn2(self.conv2(h)))
        return self.relu(self.bn3(self.conv3(h)) + x) * self.gain


def test_fuse_residual_rewrites_verifies_and_restores_on_the_cpu():
    torch.manual_seed(5)
    m = nn.Sequential(_Bottleneck(), _Bottleneck(gain=2.0), _Bottleneck()).eval()   # the second one does more than its names say
    x = torch.randn(2, 8, 5, 7)
    forwards = []
    m.register_forward_hook(lambda mod, inp, out: forwards.append(1))
    with torch.no_grad():
        y0 = m(x)
        before = _state(m)
        del forwards[:]
        assert fusion.fuse_residual(m, x) == 2 and len(forwards) == 2   # the trace and the verification of the whole model
        assert [b.__dict__.get("_residual_fused", False) for b in m] == [True, False, True]
        assert "forward" not in m[1].__dict__ and not m[1].conv3.residual_relu and "_in_residual" not in m[1].conv3.__dict__
        assert torch.equal(m(x), y0)
        assert fusion.unfuse_residual(m) == 2 and _state(m) == before
    m._forward_hooks.clear()
    assert _hooks(m) == 0
