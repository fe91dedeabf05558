"""Shared by test_bn_train_host.py and test_gpu_bn_train.py: the cases, the float64 references and a float32 NumPy model of the
order in which csrc/bn_train.hip sums (include/slfp.h states it).  Everything here runs on the CPU."""
import ctypes
import functools

import numpy as np
import torch

from cnns_slfp_quantization_amd import _lib

EPS = 1e-5
MOMENTUM = 0.1
OFFSET = 1000.0   # the offset case: mu = OFFSET * sigma (the value the issue names; the CPU pre-check holds at it)
FIXED = [(2, 5, 7, 32), (3, 1, 1, 64), (4, 9, 3, 58), (2, 3, 3, 1024), (5, 7, 3, 6)]   # (N, H, W, C)


def split(m, c):
    """(rows per slab, slabs) of slfp_debug_bn_split."""
    r, s = ctypes.c_int64(), ctypes.c_int64()
    assert _lib.load().slfp_debug_bn_split(m, c, ctypes.byref(r), ctypes.byref(s)) == _lib.OK
    return r.value, s.value


@functools.lru_cache(None)
def ragged(c):
    """The smallest (2, h, h, c) whose rows are cut into at least 3 slabs with a shorter last one."""
    for h in range(2, 200):
        m = 2 * h * h
        r, s = split(m, c)
        if s >= 3 and m % r:
            return (2, h, h, c)
    raise AssertionError("no ragged shape found")


def shapes():
    return FIXED + [ragged(32), ragged(6)]   # one vector (C % 4 == 0), one scalar


def case_id(case):
    shape, offset = case
    return "x".join(map(str, shape)) + ("-offset" if offset else "")


def cases():
    return [(s, False) for s in shapes()] + [(ragged(32), True)]


@functools.lru_cache(None)
def inputs(shape, offset):
    """x = randn * sigma_c + mu_c (channels_last, float32), |mu_c / sigma_c| <= 3, or mu = OFFSET * sigma in the offset case; gamma, beta, the
    running statistics and two upstream gradients (dense, 90 % zeros).  Cached: the tests share them and must not write to them."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(1000 + sum(shape) + (7 if offset else 0))
    sigma = torch.rand(c, generator=g) * 1.5 + 0.5
    ratio = torch.full((c,), OFFSET) if offset else torch.rand(c, generator=g) * 6 - 3
    x = torch.randn(n, c, h, w, generator=g) * sigma.view(1, c, 1, 1) + (ratio * sigma).view(1, c, 1, 1)
    x = x.contiguous(memory_format=torch.channels_last)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g)
    # an earlier running mean on the data's own scale (half the channel's mu): a running value's own float32 rounding, 2^-24 |rm| per
    # update, then stays far inside the mean bar, which is measured in units of mean|x| >= |mean x|
    rm, rv = 0.5 * ratio * sigma, torch.rand(c, generator=g) + 0.5
    gy = torch.randn(n, c, h, w, generator=g).contiguous(memory_format=torch.channels_last)
    sparse = (gy * (torch.rand(n, c, h, w, generator=g) < 0.1)).contiguous(memory_format=torch.channels_last)
    return dict(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, gy=gy, gy_sparse=sparse)


def rows(t):
    """[M, C] float64 view of an (N, C, H, W) tensor's values, rows in NHWC order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().numpy()


def forward64(x, gamma, beta, relu):
    """The textbook formulas in float64 on the float32 values: mean, biased var, y ([M, C])."""
    xr = rows(x)
    mean = xr.mean(axis=0)
    var = ((xr - mean) ** 2).mean(axis=0)
    y = (xr - mean) / np.sqrt(var + EPS) * gamma.double().numpy() + beta.double().numpy()
    return mean, var, (np.maximum(y, 0.0) if relu else y)


def running64(rm, rv, mean, var, m, calls):
    rm, rv = rm.double().numpy().copy(), rv.double().numpy().copy()
    for _ in range(calls):
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * var * m / (m - 1)
    return rm, rv


def backward64(x, g, gamma):
    """g: [M, C] float64, already masked.  Returns gx [M, C], ggamma, gbeta and the sums of |terms| of the two reductions."""
    xr = rows(x)
    m = xr.shape[0]
    mean = xr.mean(axis=0)
    invstd = 1.0 / np.sqrt(((xr - mean) ** 2).mean(axis=0) + EPS)
    xh = (xr - mean) * invstd
    gbeta, ggamma = g.sum(axis=0), (g * xh).sum(axis=0)
    gx = gamma.double().numpy() * invstd * (g - gbeta / m - xh * ggamma / m)
    return gx, ggamma, gbeta, np.abs(g * xh).sum(axis=0), np.abs(g).sum(axis=0)


def mean_bar_ok(got, mean64, x):
    """|d| <= 2 (M + 1) 2^-24 mean64(|x|): the any-order float32 summation bound of fusion._avgpool_bound_ok."""
    xr = rows(x)
    bound = 2.0 * (xr.shape[0] + 1) * 2.0 ** -24 * np.abs(xr).mean(axis=0)
    return bool((np.abs(np.asarray(got, dtype=np.float64) - mean64) <= bound).all())


def var_bar_ok(got, var64, tol):
    return bool((np.abs(np.asarray(got, dtype=np.float64) - var64) <= tol * var64).all())


def rows32(t):
    """[M, C] float32 view of an (N, C, H, W) tensor's values, rows in NHWC order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def lane_rows(m, c):
    """(R, S, TY) of include/slfp.h's split: S slabs of R rows, TY row lanes per slab."""
    r, s = split(m, c)
    groups = c // 4 if c % 4 == 0 else c
    tx = 1
    while tx < 64 and tx < groups:
        tx *= 2
    return r, s, 256 // tx


def kernel_order_forward(x, gamma, beta, save_mean, save_invstd, relu):
    """y [M, C] float32 as include/slfp.h states the apply pass, from the device's save_mean and save_invstd (float32 arrays):
    lo = f32(mean64 - f64(save_mean)) with kernel_order_stats' float64 mean, every other operation float32 and rounded on its own."""
    f32 = np.float32
    xr = rows32(x)
    save_mean, save_invstd = np.asarray(save_mean, f32), np.asarray(save_invstd, f32)
    lo = (kernel_order_stats(x)[0] - save_mean.astype(np.float64)).astype(f32)
    sc = save_invstd * gamma.numpy()
    y = (((xr - save_mean) - lo) * sc) + beta.numpy()
    assert y.dtype == f32
    return np.where(y < 0, f32(0), y) if relu else y   # a NaN and a -0.0 stay


def kernel_order_backward(x, gy, y, gamma, save_mean, save_invstd, relu):
    """(gx [M, C], ggamma, gbeta) float32 as include/slfp.h states the backward: lane partials of sg, sx, sd from +0.0f over rows
    r0 + ty, r0 + ty + TY, ..., lanes added ty ascending in float32, slabs in float64 in slab order, the finalize step in float64
    with its float32 roundings, then gx.  y is the forward's output [M, C] (the ReLU's mask; unused with relu false)."""
    f32, f64 = np.float32, np.float64
    xr, g = rows32(x), rows32(gy)
    m, c = xr.shape
    save_mean, save_invstd = np.asarray(save_mean, f32), np.asarray(save_invstd, f32)
    if relu:
        g = np.where(np.asarray(y, f32) > 0, g, f32(0))
    d = xr - save_mean
    terms = (g, g * (d * save_invstd), d)
    r, s, ty = lane_rows(m, c)
    tot = [np.zeros(c, f64) for _ in terms]   # SG, SX, SD
    for j in range(s):
        r0, r1 = j * r, min((j + 1) * r, m)
        for t, term in zip(tot, terms):
            lanes = np.zeros((ty, c), f32)
            for i in range(r0, r1, ty):       # one row per lane at a time
                k = min(ty, r1 - i)
                lanes[:k] = lanes[:k] + term[i:i + k]
            a = lanes[0].copy()
            for q in range(1, ty):
                a = a + lanes[q]
            assert a.dtype == f32
            t += a.astype(f64)
    sg, sx, sd = tot
    lo = sd / m
    sx = sx - (lo * save_invstd.astype(f64)) * sg
    gbeta, ggamma = sg.astype(f32), sx.astype(f32)
    mb, mg, lo = (sg / m).astype(f32), (sx / m).astype(f32), lo.astype(f32)
    a = gamma.numpy() * save_invstd
    xh = ((xr - save_mean) - lo) * save_invstd
    gx = a * ((g - mb) - (xh * mg))
    assert gx.dtype == f32
    return gx, ggamma, gbeta


def kernel_order_stats(x):
    """(mean, biased var) as float64, summed in float32 in the kernel's order: V, TX, TY and the slabs as include/slfp.h states
    them, lane partials from +0.0f over rows r0 + ty, r0 + ty + TY, ..., lanes added ty ascending, slabs by Chan in float64."""
    n, c, h, w = x.shape
    xr = rows32(x)
    m = xr.shape[0]
    r, s, ty = lane_rows(m, c)
    f32 = np.float32
    cnt, mean, m2 = 0.0, np.zeros(c), np.zeros(c)
    for j in range(s):
        xs = xr[j * r:min((j + 1) * r, m)]
        k = xs[0]
        s1, s2 = np.zeros((ty, c), f32), np.zeros((ty, c), f32)
        for i in range(xs.shape[0]):
            d = xs[i] - k
            s1[i % ty] = s1[i % ty] + d
            s2[i % ty] = s2[i % ty] + d * d
        a1, a2 = s1[0].copy(), s2[0].copy()
        for t in range(1, ty):
            a1 = a1 + s1[t]
            a2 = a2 + s2[t]
        assert a1.dtype == f32 and a2.dtype == f32
        nb = float(xs.shape[0])
        mb = k.astype(np.float64) + a1.astype(np.float64) / nb
        qb = a2.astype(np.float64) - a1.astype(np.float64) ** 2 / nb
        nt = cnt + nb
        delta = mb - mean
        mean = mean + delta * (nb / nt)
        m2 = (m2 + qb) + (delta * delta) * (cnt * nb / nt)
        cnt = nt
    return mean, np.maximum(m2 / m, 0.0)
