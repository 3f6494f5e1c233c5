"""Seeded inputs of the per-element gradient tests (tests/test_grad_oracle64_host.py, tests/test_gpu_grad_oracle64.py), all built
on the CPU.  Not a conftest: test modules import it.

Flow families: a smooth flow (sigma 3); the same flow shifted by (+0.6 W, -0.6 H) and by (-0.6 W, +0.6 H), so that taps leave
each border and whole rows lie outside; an integer-valued patch (weights exactly 0 and 1, positions on cell borders); an
exactly-zero disc (the splat's occlusion rule and un-occlude fill).  The upstream gradient is randn times a smooth envelope that
spans 1e-4 ... 1, so small and large gradients sit side by side.
"""
import math

import torch
import torch.nn.functional as F

FAMILIES = ['smooth', 'shift_pos', 'shift_neg', 'integer', 'zero_disc']
SHAPES = [(2, 37, 70), (2, 64, 128), (1, 17, 68), (2, 9, 3)]        # (N, H, W): ragged tiles, exact lean tiles, one odd frame, W < 4
G_SCALE = 0.5


def smooth(n, h, w, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(n, 2, max(h // 12, 2), max(w // 12, 2), generator=g) * sigma
    return F.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True).contiguous()


def flow(family, n, h, w, seed=0):
    f = smooth(n, h, w, 3.0, 1000 + seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    if family == 'shift_pos':
        f = f + torch.tensor([0.6 * w, -0.6 * h]).view(1, 2, 1, 1)
    elif family == 'shift_neg':
        f = f + torch.tensor([-0.6 * w, 0.6 * h]).view(1, 2, 1, 1)
    elif family == 'integer':
        f[:, :, h // 4:h // 4 + max(h // 2, 2), w // 4:w // 4 + max(w // 2, 1)] = \
            torch.round(f[:, :, h // 4:h // 4 + max(h // 2, 2), w // 4:w // 4 + max(w // 2, 1)])
        f[:, :, 0, :] = torch.round(f[:, :, 0, :]) - 1.0                 # a whole row of integer positions across the top border
    elif family == 'zero_disc':
        r = max(min(h, w) / 4.0, 1.5)
        f = f * (torch.sqrt((ys - h / 2.5) ** 2 + (xs - w / 2.0) ** 2) > r).float()
    else:
        assert family == 'smooth', family
    return f.contiguous()


def envelope(h, w):
    """Smooth, 1e-4 at one corner to 1 at the opposite one."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    t = (ys / max(h - 1, 1) + xs / max(w - 1, 1)) / 2.0
    return torch.exp(math.log(1e-4) * (1.0 - t))


def upstream(n, c, h, w, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return (torch.randn(n, c, h, w, generator=g) * envelope(h, w)).contiguous()


def image(n, c, h, w, seed=0):
    g = torch.Generator().manual_seed(3000 + seed)
    return (torch.rand(n, c, h, w, generator=g) * 2.0 - 0.5).contiguous()


def holes(n, h, w, seed=0):
    g = torch.Generator().manual_seed(4000 + seed)
    m = torch.rand(n, h, w, generator=g) > 0.1
    m[:, h // 2:h // 2 + max(h // 6, 1), w // 5:w // 5 + max(w // 6, 1)] = False
    return m


def points(n, h, w, m=257, seed=0):
    """M points (y, x): uniform, the four frame corners, exact integers, points outside (near and far), one NaN row, and 64 points
    in one cell."""
    g = torch.Generator().manual_seed(5000 + seed)
    size = torch.tensor([h - 1.0, w - 1.0])
    corners = torch.tensor([[0.0, 0.0], [0.0, w - 1.0], [h - 1.0, 0.0], [h - 1.0, w - 1.0]]).expand(n, 4, 2)
    cell = torch.tensor([float(h // 2), float(min(w // 2, w - 2))]) + torch.rand(n, 64, 2, generator=g) * 0.999
    ints = torch.floor(torch.rand(n, 32, 2, generator=g) * (size + 1))
    near = torch.cat([-torch.rand(n, 16, 2, generator=g) * 0.9, size + torch.rand(n, 16, 2, generator=g) * 0.9], 1)
    far = (torch.rand(n, 16, 2, generator=g) - 0.5) * 4 * size
    nan = torch.full((n, 1, 2), float('nan'))
    nan[..., 1] = 1.5
    k = m - (4 + 64 + 32 + 32 + 16 + 1)
    pts = torch.cat([corners, cell, ints, near, far, nan, torch.rand(n, k, 2, generator=g) * size], 1)
    assert pts.shape[1] == m
    return pts[:, torch.randperm(m, generator=g)].contiguous()
