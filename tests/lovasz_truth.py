"""The Lovasz-Softmax criterion in numpy, written from its definition in include/pvcnn_hip.h ("The Lovasz-Softmax criterion").  Not a
test: tests/test_lovasz_host.py and tests/test_gpu_lovasz.py hold the composition and the kernels to it.

float32 only where the definition says so (the error e = fg ? 1.0f - p : p, ONE fp32 subtraction, when the probabilities are fp32),
np.lexsort((index, -e)) for the order (e descending, ties by ascending index), fp64 for everything after."""
import numpy as np


def softmax64(x):
    """fp64 softmax over axis 1 of (B, C, S) logits."""
    x = np.asarray(x, dtype=np.float64)
    z = np.exp(x - x.max(axis=1, keepdims=True))
    return z / z.sum(axis=1, keepdims=True)


def steps(fg_sorted):
    """The steps of the Jaccard index along a list whose foreground flags, in ranked order, are fg_sorted: closed form, fp64."""
    fg_sorted = np.asarray(fg_sorted, dtype=bool)
    n = fg_sorted.size
    g = int(fg_sorted.sum())
    cf = np.cumsum(fg_sorted).astype(np.int64)
    i = np.arange(1, n + 1, dtype=np.int64)
    inter, union = g - cf, g + i - cf
    out = np.zeros(n, dtype=np.float64)
    out[fg_sorted] = 1.0 / union[fg_sorted]
    bg = ~fg_sorted & (union > 1)
    out[bg] = inter[bg] / (union[bg].astype(np.float64) * (union[bg] - 1))
    if g == 0 and n > 0:
        out[0] = 1.0
    return out


def jaccard_differences(fg_sorted):
    """The same steps as differences of the Jaccard index 1 - I / U in fp64 (what the closed form replaces)."""
    fg_sorted = np.asarray(fg_sorted, dtype=bool)
    g = int(fg_sorted.sum())
    cf = np.cumsum(fg_sorted).astype(np.float64)
    i = np.arange(1, fg_sorted.size + 1, dtype=np.float64)
    jac = 1.0 - (g - cf) / (g + i - cf)
    return np.diff(np.concatenate([[0.0], jac]))


def list_loss(e, fg):
    """One list: errors e (their own dtype) and foreground flags of its live points -> (loss fp64, d loss / d e fp64, in the
    points' order)."""
    e, fg = np.asarray(e), np.asarray(fg, dtype=bool)
    order = np.lexsort((np.arange(e.size), -e))
    st = steps(fg[order])
    grad = np.zeros(e.size, dtype=np.float64)
    grad[order] = st
    return float(np.sum(e[order].astype(np.float64) * st)), grad


def lovasz_softmax(p, t, classes='present', ignore_index=-100):
    """p (B, C, S) probabilities (fp32: the errors are fp32 subtractions; fp64: fp64 ones), t (B, S) integers ->
    (loss fp64, d loss / d p fp64 (B, C, S), number of out-of-range targets)."""
    p, t = np.asarray(p), np.asarray(t)
    B, C, S = p.shape
    one = p.dtype.type(1.0)
    grad = np.zeros((B, C, S), dtype=np.float64)
    clouds = np.zeros(B, dtype=np.float64)
    in_range = (t >= 0) & (t < C)
    live_all = (t != ignore_index) & in_range
    bad = int(((t != ignore_index) & ~in_range).sum())
    for b in range(B):
        live = live_all[b]
        idx = np.nonzero(live)[0]
        losses, grads, counted = [], [], []
        for c in range(C):
            fg = t[b, idx] == c
            if (classes == 'present' and not fg.any()) or idx.size == 0:
                continue
            pc = p[b, c, idx]
            e = np.where(fg, one - pc, pc)
            assert e.dtype == p.dtype
            loss, g = list_loss(e, fg)
            losses.append(loss)
            grads.append(np.where(fg, -g, g))
            counted.append(c)
        if counted:
            clouds[b] = sum(losses) / len(counted)
            for c, g in zip(counted, grads):
                grad[b, c, idx] = g / (len(counted) * B)
    return float(clouds.sum() / B), grad, bad


def logits_gradient(p, grad_p):
    """The softmax Jacobian in fp64: dx_j = p_j (g_j - sum_c p_c g_c) on (B, C, S)."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(grad_p, dtype=np.float64)
    return p * (g - (p * g).sum(axis=1, keepdims=True))
