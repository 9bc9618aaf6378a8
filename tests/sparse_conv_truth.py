"""The truth of the sparse voxel operators (include/pvcnn_hip.h, "Sparse voxels"), in plain torch fp64 on the CPU and plain Python:

    truth_map      voxel / index / offsets / nbr by a Python loop over a dictionary of coordinates
    truth_conv     rows scattered into a zero grid, F.conv3d(padding = 1), read at the active voxels, the bias only there
    truth_grads    the three gradients by autograd of that composition
    brute_conv     the definition as a triple loop (for the smallest grids: pins truth_conv itself)

and the clouds of the test cases (`make_cnt`).  Nothing here imports the package under test."""
import torch
import torch.nn.functional as TF


def taps():
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]       # nn.Conv3d's order: tap 13 = (0, 0, 0)


def truth_map(cnt, r, cap=None):
    """cnt (B, R^3) -> dict(voxel, index, offsets, nbr, count, total): int64 tensors, the rows ascending in the flat voxel number."""
    cnt = cnt.detach().cpu()
    b, r3 = cnt.shape[0], r ** 3
    coords = {}                                    # (b, x, y, z) -> row
    voxel, offsets = [], []
    flat = cnt.reshape(-1).tolist()
    total = sum(1 for c in flat if c > 0)
    cap = total if cap is None else cap
    for bi in range(b):
        offsets.append(len(voxel))                 # the first row of the cloud (never above cap)
        for s in range(r3):
            if flat[bi * r3 + s] > 0 and len(voxel) < cap:
                coords[(bi, s // (r * r), (s // r) % r, s % r)] = len(voxel)
                voxel.append(bi * r3 + s)
    count = len(voxel)
    offsets.append(count)
    index = [-1] * (b * r3)
    for row, v in enumerate(voxel):
        index[v] = row
    nbr = [[-1] * 27 for _ in range(cap)]
    for (bi, x, y, z), row in coords.items():
        for tap, (dx, dy, dz) in enumerate(taps()):
            nbr[row][tap] = coords.get((bi, x + dx, y + dy, z + dz), -1)          # a key outside [0, R) or of another cloud is absent
    return dict(voxel=torch.tensor(voxel + [-1] * (cap - count), dtype=torch.int64), index=torch.tensor(index, dtype=torch.int64),
                offsets=torch.tensor(offsets, dtype=torch.int64), nbr=torch.tensor(nbr, dtype=torch.int64).reshape(cap, 27),
                count=count, total=total, cap=cap, batch=b, r=r)


def _scatter(rows, m):
    b, r = m['batch'], m['r']
    v = m['voxel'][:m['count']]
    g = rows.new_zeros((b, r ** 3, rows.shape[1]))
    g = g.index_put((v // r ** 3, v % r ** 3), rows[:m['count']])
    return g.permute(0, 2, 1).reshape(b, rows.shape[1], r, r, r)


def _gather(grid, m):
    b, r = m['batch'], m['r']
    v = m['voxel'][:m['count']]
    g = grid.reshape(b, grid.shape[1], -1)
    return torch.cat([g[v // r ** 3, :, v % r ** 3], g.new_zeros((m['cap'] - m['count'], grid.shape[1]))], 0)


def truth_scatter(rows, m):
    return _scatter(rows.detach().cpu().double(), m)


def truth_gather(grid, m):
    return _gather(grid.detach().cpu().double(), m)


def _conv(rows, weight, bias, m):
    y = _gather(TF.conv3d(_scatter(rows, m), weight, None, padding=1), m)
    if bias is not None:
        live = (torch.arange(m['cap']) < m['count']).to(y.dtype)
        y = y + live[:, None] * bias[None, :]
    return y


def truth_conv(rows, weight, bias, m):
    """-> y (cap, Co) fp64; the rows >= count are never read (they may hold NaN) and come out as zeros."""
    x = rows.detach().cpu().double().clone()
    x[m['count']:] = 0
    return _conv(x, weight.detach().cpu().double(), None if bias is None else bias.detach().cpu().double(), m)


def truth_grads(rows, weight, bias, grad_y, m):
    """-> (grad_rows, grad_weight, grad_bias) fp64 by autograd of truth_conv's composition; grad_y's rows >= count are not read."""
    x = rows.detach().cpu().double().clone()
    x[m['count']:] = 0
    x.requires_grad_()
    w = weight.detach().cpu().double().clone().requires_grad_()
    bb = None if bias is None else bias.detach().cpu().double().clone().requires_grad_()
    gy = grad_y.detach().cpu().double().clone()
    gy[m['count']:] = 0
    y = _conv(x, w, bb, m)
    y.backward(gy)
    return x.grad, w.grad, None if bb is None else bb.grad


def brute_conv(rows, weight, bias, m):
    """The definition as loops: y[j, co] = bias[co] + sum_tap sum_ci W[co, ci, tap] x[nbr[j, tap], ci]."""
    x, w = rows.detach().cpu().double(), weight.detach().cpu().double().reshape(weight.shape[0], weight.shape[1], 27)
    y = torch.zeros((m['cap'], w.shape[0]), dtype=torch.float64)
    for j in range(m['count']):
        for co in range(w.shape[0]):
            s = 0.0 if bias is None else float(bias[co])
            for tap in range(27):
                n = int(m['nbr'][j, tap])
                if n >= 0:
                    for ci in range(w.shape[1]):
                        s += float(w[co, ci, tap]) * float(x[n, ci])
            y[j, co] = s
    return y


# ---- the clouds of the test cases: name -> (B, R, Ci, Co) and the counts
CASES = {'a': (1, 1, 1, 1), 'b': (2, 4, 5, 7), 'c': (3, 8, 9, 64), 'd': (2, 16, 64, 64), 'e': (1, 32, 16, 130)}


def make_cnt(case, seed=1588147245):
    """-> cnt (B, R^3) int32 of a case.  a: one voxel.  b: every voxel active.  c: about 20 % occupancy, the middle cloud EMPTY, voxel
    (7, 7, 7) of cloud 0 and (0, 0, 0) of cloud 2 active (adjacent rows across a cloud boundary), and a run of voxels across the end
    of a z row of cloud 0: (3, 2, 5..7) and (3, 3, 0..2).  d: 300 points per cloud.  e: 4096 points."""
    b, r, _, _ = CASES[case]
    g = torch.Generator().manual_seed(seed + ord(case))
    cnt = torch.zeros((b, r, r, r), dtype=torch.int32)
    if case == 'a':
        cnt[:] = 3
    elif case == 'b':
        cnt[:] = torch.randint(1, 4, cnt.shape, generator=g, dtype=torch.int32)
    elif case == 'c':
        cnt[:] = (torch.rand(cnt.shape, generator=g) < 0.2).to(torch.int32) * 2
        cnt[1] = 0
        cnt[0, 7, 7, 7] = 1
        cnt[2, 0, 0, 0] = 1
        cnt[0, 3, 2, 5:8] = 1
        cnt[0, 3, 3, 0:3] = 1
    else:
        n = 300 if case == 'd' else 4096
        for bi in range(b):                        # points on a wavy surface, like a scanned room: clustered, many per voxel
            u = torch.rand((n, 2), generator=g)
            h = 0.5 + 0.25 * torch.sin(6.0 * u[:, 0]) * torch.cos(5.0 * u[:, 1]) + 0.02 * torch.rand((n,), generator=g)
            p = (torch.stack([u[:, 0], u[:, 1], h], 1) * r).long().clamp(0, r - 1)
            cnt[bi].index_put_((p[:, 0], p[:, 1], p[:, 2]), torch.ones((n,), dtype=torch.int32), accumulate=True)
    return cnt.reshape(b, r ** 3)
