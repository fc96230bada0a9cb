"""The per-system L-BFGS mode for ONE system, stated in float64 torch from its contract (include/adsorbdiff_hip.h,
``adf_lbfgs_set_per_system``): own step counter, own deque of (s, y, rho), dot products over the system's 3 n entries,
own skip decision.  Shared by the CPU and the GPU tests of the mode."""
from collections import deque

import torch


def max_force(f):
    """check_convergence's max |f_atom| of one system in f64 (NaN propagates, as torch's max does)."""
    f = torch.as_tensor(f).to(torch.float64).reshape(-1, 3)
    return (f ** 2).sum(1).sqrt().max() if f.shape[0] else torch.zeros((), dtype=torch.float64)


class OneSystemLBFGS:
    def __init__(self, memory, maxstep=0.04, damping=1.0, alpha=70.0):
        self.memory, self.maxstep, self.damping, self.H0 = int(memory), float(maxstep), float(damping), 1.0 / float(alpha)
        self.t = 0
        self.s, self.y, self.rho = deque(maxlen=self.memory), deque(maxlen=self.memory), deque(maxlen=self.memory)
        self.r0 = self.f0 = None
        self.last_absmax = -1.0   # of the last call: -1 = no step attempted

    def step(self, pos, forces, mask_set):
        """pos f32 [n, 3] (updated in place), forces f32 [n, 3] with the constraint applied; returns True when the step was
        skipped, False when it moved the system, None when the mask was clear."""
        if not mask_set:
            self.last_absmax = -1.0
            return None
        r = pos.detach().cpu().to(torch.float64).reshape(-1)
        f = forces.detach().cpu().to(torch.float64).reshape(-1)
        if self.t > 0:
            s0, y0 = r - self.r0, -(f - self.f0)
            self.s.append(s0)
            self.y.append(y0)
            self.rho.append(1.0 / torch.dot(y0, s0))
        loopmax = min(self.memory, self.t)
        a = [None] * loopmax
        q = -f
        for i in range(loopmax - 1, -1, -1):
            a[i] = self.rho[i] * torch.dot(self.s[i], q)
            q = q - a[i] * self.y[i]
        z = self.H0 * q
        for i in range(loopmax):
            beta = self.rho[i] * torch.dot(self.y[i], z)
            z = z + self.s[i] * (a[i] - beta)
        p = -z.reshape(-1, 3)
        longest = p.norm(dim=1).max()
        scale = (longest + 1e-7).reciprocal() * torch.minimum(longest, longest.new_tensor(self.maxstep))
        dr = p * scale * self.damping
        absmax = dr.abs().max()
        self.last_absmax = float(absmax)
        self.t += 1
        if bool(absmax < 1e-7):   # False for NaN: a NaN does not skip
            return True
        pos.add_(dr.to(torch.float32).reshape(pos.shape).to(pos.device))
        self.r0, self.f0 = r, f
        return False


def ulp_close(a, b, ulps=1):
    """Every element of ``a`` within ``ulps`` float32 ulps (of ``b``) of ``b``."""
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    up = (torch.nextafter(b.abs(), torch.full_like(b, float("inf"))) - b.abs()) * ulps
    return bool(((a - b).abs() <= up).all())


def split_systems(x, natoms):
    """Rows of a per-atom tensor, system by system."""
    return list(torch.split(torch.as_tensor(x), [int(n) for n in natoms]))
