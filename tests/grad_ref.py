"""The reference's differentiable op sequences, restated with torch ops on tensors (autograd through F.grid_sample and
scatter_add_), for the gradient tests.  Not a conftest: test modules import it.

Each function mirrors the body of the reference function it names (PURE_PYTORCH branches, float targets), line for line
and in the same fp32 operation order, so that on the CPU its forward values are the reference's own and its gradients are
what the reference's autograd computes.  tests/test_grad_ref_golden.py pins it to the committed fixtures (grads.*,
next.track_pts_*, next.*get_padding*); the GPU tier (tests/test_gpu_gradients.py) then uses it as the reference at frame
sizes where no fixture exists.

`RFlow` is a tensor-level stand-in for the reference's Flow class: vecs [N,2,H,W], ref, mask [N,H,W].
"""
import numpy as np
import torch
import torch.nn.functional as F

DEFAULT_THRESHOLD = 1e-3                                                       # utils.py:23


# ------------------------------------------------------------------------------------------------
# utils.py
# ------------------------------------------------------------------------------------------------
def threshold_vectors(vecs, threshold=None):
    """utils.py:623-643 (use_mag False)."""
    threshold = DEFAULT_THRESHOLD if threshold is None else threshold
    f = vecs.clone()
    f[(vecs < threshold) & (vecs > -threshold)] = 0
    return f


def is_zero_flow(flow, thresholded=True):
    """utils.py:922-938."""
    f = threshold_vectors(flow) if thresholded else flow
    return torch.sum(f == 0, (1, 2, 3)) == f[0].numel()


def normalise_coords(coords, shape):
    """utils.py:446-466."""
    normalised_coords = coords.float() * 2
    normalised_coords[..., 0] /= (shape[1] - 1)
    normalised_coords[..., 1] /= (shape[0] - 1)
    normalised_coords -= 1
    return normalised_coords


def get_flow_endpoints(flow, ref):
    """utils.py:1045-1059."""
    n, _, h, w = flow.shape
    s = +1 if ref == 's' else -1
    x = s * flow[:, 0] + torch.arange(w, device=flow.device)[None, None, :]
    y = s * flow[:, 1] + torch.arange(h, device=flow.device)[None, :, None]
    return x, y


def grid_from_unstructured_data(x, y, data, mask=None):
    """utils.py:1062-1144."""
    n, c, h, w = data.shape
    x0, y0 = torch.floor(x), torch.floor(y)
    xx, yy = torch.stack((x0, x0 + 1), dim=-1), torch.stack((y0, y0 + 1), dim=-1)
    xx_safe, yy_safe = torch.clamp(xx, min=0, max=w - 1), torch.clamp(yy, min=0, max=h - 1)
    wt_xx = torch.stack((xx[..., 1] - x, x - xx[..., 0]), dim=-1) * torch.eq(xx, xx_safe).float()
    wt_yy = torch.stack((yy[..., 1] - y, y - yy[..., 0]), dim=-1) * torch.eq(yy, yy_safe).float()
    wgt = torch.matmul(wt_yy.unsqueeze(-1), wt_xx.unsqueeze(-2))
    wgt = wgt.permute(0, 3, 4, 1, 2).reshape(n * 4, h * w)
    pos = (w * yy_safe).unsqueeze(-1) + xx_safe.unsqueeze(-2)
    pos = pos.permute(0, 3, 4, 1, 2).reshape(n * 4, h * w)
    if mask is not None:
        wgt = wgt * mask.repeat_interleave(4, dim=0).view(n * 4, h * w).to(torch.uint8)
    density = torch.zeros((n * 4, h * w), device=data.device).scatter_add(1, pos.long(), wgt)
    density = torch.sum(density.view(n, 4, h, w), dim=1, keepdim=True)
    grid_data = torch.zeros((n * 4 * c, h * w), device=data.device).scatter_add(
        1, pos.repeat_interleave(c, dim=0).long(),
        wgt.repeat_interleave(c, dim=0) * data.repeat_interleave(4, dim=0).view(n * 4 * c, h * w))
    grid_data = torch.sum(grid_data.view(n, 4, c, h, w), dim=1) / torch.clamp_min(density, 1e-3)
    return grid_data, density.squeeze(1)


def apply_s_flow(flow, data, mask=None, occlude_zero_flow=True):
    """utils.py:1157-1205: the zero-flow occlusion rule, `density > 0`, the un-occlude fill."""
    n, c, h, w = data.shape
    x, y = get_flow_endpoints(flow, 's')
    zero_mask = None
    if mask is None:
        mask = torch.ones((n, h, w), dtype=torch.bool, device=flow.device)
    if occlude_zero_flow:
        zero_mask = torch.sum(threshold_vectors(flow) == 0, dim=1) == 2
        flow_mask = mask & ~zero_mask
    else:
        flow_mask = mask
    warped_data, warped_density = grid_from_unstructured_data(x, y, data, flow_mask)
    warped_mask = (warped_density > 0).squeeze(1)
    if occlude_zero_flow:
        unocclude_mask = (mask & zero_mask & ~warped_mask).unsqueeze(1).expand(-1, c, -1, -1)
        warped_data[unocclude_mask] = data[unocclude_mask].float()
    return warped_data, warped_mask


def apply_flow(flow, target, ref, mask=None):
    """utils.py:469-555, 574-576 (float targets of shape N-C-H-W; the result keeps the float dtype)."""
    if all(is_zero_flow(flow, thresholded=True)):
        return target
    h, w = flow.shape[-2:]
    target = target.to(torch.float)
    if target.shape[0] < flow.shape[0]:
        target = target.expand(flow.shape[0], -1, -1, -1)
    elif flow.shape[0] < target.shape[0]:
        flow = flow.expand(target.shape[0], -1, -1, -1)
        if mask is not None:
            mask = mask.expand(target.shape[0], -1, -1)
    if ref == 't':
        grid_x, grid_y = torch.meshgrid(torch.arange(0, h), torch.arange(0, w), indexing='ij')
        grid = torch.stack((grid_y, grid_x), dim=-1).to(torch.float).to(flow.device)
        field = normalise_coords(grid.unsqueeze(0) - flow.permute(0, 2, 3, 1), (h, w))
        return F.grid_sample(target, field, align_corners=True)
    result, _ = apply_s_flow(flow, target, mask, occlude_zero_flow=True)
    return result


def track_pts(flow, ref, pts, int_out=False):
    """utils.py:941-1042 (PURE_PYTORCH): float points through grid_sample, integer points through gather."""
    return_2d = False
    if pts.dim() == 2:
        return_2d = True
        pts = pts.unsqueeze(0).expand(flow.shape[0], -1, -1)
    elif pts.shape[0] != flow.shape[0]:
        pts = pts.expand(flow.shape[0], -1, -1)
    if all(is_zero_flow(flow, thresholded=True)):
        warped_pts = pts
    else:
        if ref == 't':
            x, y = get_flow_endpoints(-flow, 's')
            flow, _ = grid_from_unstructured_data(x, y, flow)
        if not pts.dtype.is_floating_point:
            flow_vecs = flow.permute(0, 2, 3, 1)
            pts2 = pts[..., 0] * flow.shape[-1] + pts[..., 1]
            pts2 = pts2.unsqueeze(-1).expand(-1, -1, 2)
            flow_vecs = torch.gather(flow_vecs.reshape(flow_vecs.shape[0], -1, 2), 1, pts2.long())
            flow_vecs = flow_vecs.flip(-1)
        else:
            pts_4d = normalise_coords(pts.unsqueeze(1).to(torch.float).flip(-1), flow.shape[-2:])
            flow_vecs = F.grid_sample(flow, pts_4d, align_corners=True).flip(1)
            flow_vecs = flow_vecs.squeeze(2).permute(0, 2, 1)
        warped_pts = pts.float() + flow_vecs
        nan_vals = torch.isnan(warped_pts)
        nan_vals = nan_vals[:, :, 0] | nan_vals[:, :, 1]
        warped_pts[nan_vals] = 0
    if int_out:
        warped_pts = torch.round(warped_pts).long()
    if return_2d:
        warped_pts = warped_pts.squeeze(0)
    return warped_pts


def _ref_apply_t(flow, target):
    """utils.py:541-555 restated with torch ops on the operands' device (autograd through grid_sample)."""
    n, _, h, w = flow.shape
    gy, gx = torch.meshgrid(torch.arange(h, device=flow.device), torch.arange(w, device=flow.device), indexing='ij')
    grid = torch.stack((gx, gy), dim=-1).float().unsqueeze(0)
    field = (grid - flow.permute(0, 2, 3, 1)) * 2
    field = torch.stack((field[..., 0] / (w - 1), field[..., 1] / (h - 1)), dim=-1) - 1
    return F.grid_sample(target.expand(n, -1, -1, -1), field, align_corners=True)


def _ref_splat(x, y, data, mask):
    """utils.py:1098-1144 restated with torch ops on the operands' device (autograd through the weights and scatter_add_)."""
    n, c, h, w = data.shape
    x0, y0 = torch.floor(x), torch.floor(y)
    xx, yy = torch.stack((x0, x0 + 1), -1), torch.stack((y0, y0 + 1), -1)
    xs, ys = torch.clamp(xx, 0, w - 1), torch.clamp(yy, 0, h - 1)
    wx = torch.stack((xx[..., 1] - x, x - xx[..., 0]), -1) * torch.eq(xx, xs).float()
    wy = torch.stack((yy[..., 1] - y, y - yy[..., 0]), -1) * torch.eq(yy, ys).float()
    wgt = torch.matmul(wy.unsqueeze(-1), wx.unsqueeze(-2)).permute(0, 3, 4, 1, 2).reshape(n * 4, h * w)
    pos = ((w * ys).unsqueeze(-1) + xs.unsqueeze(-2)).permute(0, 3, 4, 1, 2).reshape(n * 4, h * w)
    if mask is not None:
        wgt = wgt * mask.repeat_interleave(4, dim=0).view(n * 4, h * w).float()
    den = torch.zeros((n * 4, h * w), device=data.device).scatter_add(1, pos.long(), wgt)
    den = den.view(n, 4, h, w).sum(1, keepdim=True)
    acc = torch.zeros((n * 4 * c, h * w), device=data.device).scatter_add(
        1, pos.repeat_interleave(c, dim=0).long(), wgt.repeat_interleave(c, dim=0) * data.repeat_interleave(4, dim=0).view(n * 4 * c, h * w))
    return acc.view(n, 4, c, h, w).sum(1) / torch.clamp_min(den, 1e-3), den.squeeze(1)


# ------------------------------------------------------------------------------------------------
# flow_class.py
# ------------------------------------------------------------------------------------------------
class RFlow(object):
    """The reference's Flow, reduced to what its differentiable methods read: vecs [N,2,H,W], ref, mask [N,H,W] bool."""

    def __init__(self, vecs, ref='t', mask=None):
        self.vecs = vecs
        self.ref = ref
        n, _, h, w = vecs.shape
        if mask is None:
            mask = torch.ones(n, h, w, dtype=torch.bool, device=vecs.device)
        elif mask.dim() == 2:
            mask = mask.unsqueeze(0)
        self.mask = mask.to(torch.bool).to(vecs.device)

    @property
    def shape(self):
        return (self.vecs.shape[0],) + tuple(self.vecs.shape[2:])

    def __add__(self, other):                                                  # flow_class.py:450-488
        if isinstance(other, RFlow):
            return RFlow(self.vecs + other.vecs, self.ref, self.mask & other.mask)
        return RFlow(self.vecs + other, self.ref, self.mask)

    def __sub__(self, other):                                                  # :490-531
        if isinstance(other, RFlow):
            return RFlow(self.vecs - other.vecs, self.ref, self.mask & other.mask)
        return RFlow(self.vecs - other, self.ref, self.mask)

    def __mul__(self, other):                                                  # :549 (scalars)
        return RFlow(self.vecs * float(other), self.ref, self.mask)

    def __neg__(self):                                                         # :680-692
        return self * -1

    def select(self, item=None):                                               # :413-430
        if item is None:
            return self
        return RFlow(self.vecs[item:item + 1], self.ref, self.mask[item:item + 1])

    def pad(self, padding, mode='constant'):                                   # :715-736
        padded_vecs = F.pad(self.vecs, (*padding[2:], *padding[:2]), mode=mode)
        padded_mask = F.pad(self.mask.unsqueeze(1), (*padding[2:], *padding[:2])).squeeze(1)
        return RFlow(padded_vecs, self.ref, padded_mask)

    def is_zero(self, thresholded=True, masked=True):                          # :1226-1244
        f = self.vecs.clone()
        if masked:
            f[~self.mask.unsqueeze(1).expand(-1, 2, -1, -1)] = 0
        return is_zero_flow(f, thresholded)

    def apply(self, target, target_mask=None, return_valid_area=False, consider_mask=True, padding=None, cut=True):
        """flow_class.py:755-951 (float tensor targets or RFlow targets)."""
        if isinstance(target, RFlow):
            return_flow = True
            t, mask = target.vecs, target.mask
        else:
            return_flow = False
            t = target.to(torch.float)
            t_shape = (t.shape[0], *t.shape[2:])
            mask = torch.ones(t_shape, dtype=torch.bool, device=t.device) if target_mask is None else target_mask
        if return_flow or return_valid_area:
            if self.ref == 's':
                if mask.shape[-2:] != self.shape[-2:]:
                    tmp_self_mask = self.mask if self.shape[0] >= mask.shape[0] else self.mask.expand(mask.shape[0], -1, -1)
                    mask = mask.clone()
                    for i in range(mask.shape[0]):
                        m = mask[i, padding[0]:padding[0] + self.shape[1], padding[2]:padding[2] + self.shape[2]].clone()
                        mask[i, ...] = False
                        mask[i, padding[0]:padding[0] + self.shape[1], padding[2]:padding[2] + self.shape[2]] = \
                            m & tmp_self_mask[i]
                else:
                    mask = mask & self.mask
            if mask.shape[0] != t.shape[0]:
                t = t.expand(mask.shape[0], -1, -1, -1)
            t = torch.cat((t.float(), mask.unsqueeze(1).float()), dim=1)
        if padding is None:
            warped_t = apply_flow(self.vecs, t, self.ref, self.mask if consider_mask else None)
        else:
            flow = self.pad(padding, mode='constant' if self.ref == 't' else 'replicate')
            warped_t = apply_flow(flow.vecs, t, flow.ref, flow.mask if consider_mask else None)
        if padding is not None and cut:
            warped_t = warped_t[..., padding[0]:padding[0] + self.shape[1], padding[2]:padding[2] + self.shape[2]]
        if return_flow or return_valid_area:
            mask = warped_t[:, -1] > 0.99999
            if self.ref == 't':
                if mask.shape[1:] != self.mask.shape[1:]:
                    tmp = mask[:, padding[0]:padding[0] + self.shape[1], padding[2]:padding[2] + self.shape[2]].clone()
                    mask[...] = False
                    mask[:, padding[0]:padding[0] + self.shape[1], padding[2]:padding[2] + self.shape[2]] = tmp & self.mask
                else:
                    mask = mask & self.mask
        if return_flow:
            return RFlow(warped_t[:, :2, :, :], target.ref, mask)
        if return_valid_area:
            return warped_t[:, :-1, :, :], mask
        return warped_t

    def switch_ref(self):                                                      # :1022-1062 (mode 'valid')
        if all(self.is_zero(thresholded=False)):
            return RFlow(self.vecs, 't' if self.ref == 's' else 's', self.mask)
        if self.ref == 's':
            switched = self.apply(self)
            switched.ref = 't'
            return switched
        flow_copy_s = RFlow(self.vecs, 's', self.mask)
        return (-flow_copy_s).apply(flow_copy_s)

    def invert(self, ref=None):                                                # :1064-1086
        ref = self.ref if ref is None else ref
        if self.ref == 's':
            return self.apply(-self) if ref == 's' else RFlow(-self.vecs, 't', self.mask)
        return RFlow(-self.vecs, 's', self.mask) if ref == 's' else self.invert('s').switch_ref()

    def combine_with(self, flow, mode, thresholded=False):
        """flow_class.py:1740-1810 (PURE_PYTORCH branches)."""
        if all(self.is_zero(thresholded=thresholded)):
            return flow
        elif all(flow.is_zero(thresholded=thresholded)):
            return self.invert() if mode in (1, 2) else self
        if mode == 1:
            if self.ref == 's':
                flow_inv_t = flow.invert('t')
                return flow - (flow_inv_t + flow_inv_t.apply(self.switch_ref())).apply(self)
            return self.invert().apply(flow - self)
        if mode == 2:
            if self.ref == 's':
                return self.apply(flow - self)
            return flow - flow.apply(self.invert().apply(self))
        if self.ref == 's':
            return self + self.invert(ref='t').apply(flow)
        return flow + flow.apply(self)

    def combine(self, other, mode, ref=None):
        """flow_class.py:1812-1939."""
        ref = self.ref if ref is None else ref
        direction = [[0, +1, +1], [-1, 0, +1], [-1, -1, 0]]
        indices = [[1, 2], [0, 2], [0, 1]]
        timetable = [[0, 1], [1, 2], [0, 2]]
        r_time_list = [2, 0, 1]
        mode -= 1
        s_time, t_time = timetable[mode]
        g_time = timetable[mode][0 if ref == 's' else 1]
        r_time = r_time_list[mode]
        flow_ind = indices[mode]
        if (mode == 0 and g_time == s_time) or (mode in [1, 2] and g_time == t_time):
            close_input, far_input = other, self
            flow_ind = [flow_ind[1], flow_ind[0]]
        else:
            close_input, far_input = self, other
        close_time = timetable[flow_ind[0]][0 if close_input.ref == 's' else 1]
        far_time = timetable[flow_ind[1]][0 if far_input.ref == 's' else 1]
        if far_time in timetable[mode]:
            far_input = far_input.switch_ref()
        if close_time == g_time:
            if direction[r_time][g_time] == 1:
                far_input = close_input.apply(far_input)
            else:
                far_input = close_input.invert(ref='t').apply(far_input)
        if g_time == t_time:
            result = far_input * direction[s_time][r_time] + close_input * direction[r_time][t_time]
        else:
            result = close_input * direction[s_time][r_time] + far_input * direction[r_time][t_time]
        if close_time != g_time:
            if direction[r_time][g_time] == 1:
                result = close_input.apply(result)
            else:
                result = close_input.invert(ref='s').apply(result)
        result.ref = ref
        return result

    def track(self, pts, int_out=False):                                       # :1008-1010
        warped_pts = track_pts(self.vecs, self.ref, pts, int_out)
        if pts.dim() == 2 and self.shape[0] == 1:
            warped_pts = warped_pts.squeeze(0)
        return warped_pts

    def get_padding(self, item=None):
        """flow_class.py:1192-1224."""
        flow = self.select(item)
        v = threshold_vectors(flow.vecs)
        if flow.ref == 's':
            v *= -1
        grid_x, grid_y = torch.meshgrid(torch.arange(0, flow.shape[1]), torch.arange(0, flow.shape[2]), indexing='ij')
        v[:, 0] -= grid_y.to(v.device)
        v[:, 1] -= grid_x.to(v.device)
        v *= -1
        padding = []
        for i in range(flow.shape[0]):
            pad = [
                max(-torch.min(v[i, 1, flow.mask[i]]), 0),
                max(torch.max(v[i, 1, flow.mask[i]]) - (flow.shape[1] - 1), 0),
                max(-torch.min(v[i, 0, flow.mask[i]]), 0),
                max(torch.max(v[i, 0, flow.mask[i]]) - (flow.shape[2] - 1), 0)
            ]
            padding.append([int(np.ceil(float(p))) for p in pad])
        return padding[0] if item is not None else padding


def flow_padding(vecs, ref):
    """get_flow_padding (utils.py): the padding of an all-valid flow."""
    return RFlow(vecs, ref).get_padding()
