"""The default (coupled) L-BFGS mode stated in float64 torch on the CPU, the case table of the sizes at which the device's
multi-workgroup reductions change shape, and the scripted harmonic inputs of those cases.  Shared by
tests/test_relax_coupled_host.py (no GPU) and tests/test_gpu_relax_coupled.py.

``CoupledLBFGS`` restates the reference's step (relaxation/optimizers/lbfgs_torch.py:145-200): one deque of (s, y, rho),
dot products over the whole flattened batch, determine_step with the per-system longest atom step, ONE skip decision over
the batch, the masked f32 update.  The dot product is an argument, so the same code runs with another summation order
(``ShuffledDot``) or with a deliberately wrong sum (``DroppingDot``)."""
from collections import deque, namedtuple

import torch

from tests.helpers_lbfgs_per_system import max_force, split_systems, ulp_close  # noqa: F401  (re-exported for the tests)


class CoupledLBFGS:
    def __init__(self, memory, maxstep=0.04, damping=1.0, alpha=70.0, early_stop_batch=False, dot=None):
        self.memory, self.maxstep, self.damping, self.H0 = int(memory), float(maxstep), float(damping), 1.0 / float(alpha)
        self.early = bool(early_stop_batch)
        self.dot = torch.dot if dot is None else dot
        self.hist = deque(maxlen=self.memory)     # (s, y, rho): the reference's three deques move together
        self.r0 = self.f0 = None

    def step(self, it, pos, forces, batch, mask):
        """Iteration ``it`` = 0, 1, 2, ...: pos f32 [N, 3] (moved in place), forces f32 [N, 3] with the constraint applied,
        batch int64 [N] (the system of every atom, ascending), mask bool [B] (the update mask of every system).  Returns
        (z f64 [N, 3], max |dr| over the batch, skipped)."""
        batch = torch.as_tensor(batch).cpu().long()
        mask = torch.as_tensor(mask).cpu().bool()
        r = pos.detach().cpu().to(torch.float64).reshape(-1)
        f = forces.detach().cpu().to(torch.float64).reshape(-1)
        if it > 0:
            s0, y0 = r - self.r0, -(f - self.f0)
            self.hist.append((s0, y0, 1.0 / self.dot(y0, s0)))
        loopmax = min(self.memory, it)
        a = [None] * loopmax
        q = -f
        for i in range(loopmax - 1, -1, -1):
            s_i, y_i, rho_i = self.hist[i]
            a[i] = rho_i * self.dot(s_i, q)
            q = q - a[i] * y_i
        z = self.H0 * q
        for i in range(loopmax):
            s_i, y_i, rho_i = self.hist[i]
            beta = rho_i * self.dot(y_i, z)
            z = z + s_i * (a[i] - beta)
        # determine_step: every system is scaled by its own longest atom step
        p = -z.reshape(-1, 3)
        length = ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).sqrt()
        counts = torch.bincount(batch, minlength=int(mask.shape[0])).tolist()
        longest = torch.stack([c.max() if c.numel() else length.new_zeros(()) for c in torch.split(length, counts)])
        scale = (longest + 1e-7).reciprocal() * torch.minimum(longest, longest.new_tensor(self.maxstep))
        dr = p * scale[batch].unsqueeze(1) * self.damping
        absmax = dr.abs().max()
        if bool(absmax < 1e-7):   # False for NaN: a NaN does not skip.  r0 / f0 stay
            return z.reshape(-1, 3), absmax, True
        update = dr if self.early else torch.where(mask[batch].unsqueeze(1), dr, torch.zeros_like(dr))
        pos.add_(update.to(torch.float32).reshape(pos.shape).to(pos.device))
        self.r0, self.f0 = r, f
        return z.reshape(-1, 3), absmax, False


class ShuffledDot:
    """The same sum in another order: the rounded products, added one after the other in a seeded shuffled order."""

    def __init__(self, n, seed):
        self.perm = torch.randperm(int(n), generator=torch.Generator().manual_seed(seed))

    def __call__(self, a, b):
        return (a * b)[self.perm].cumsum(0)[-1]


class DroppingDot:
    """A subtly wrong reduction: dot product number ``call`` of iteration ``iteration`` (0 = the rho dot, 1 = the first
    alpha dot, ...) loses entry ``entry``.  ``begin(it)`` before every step."""

    def __init__(self, iteration, call, entry):
        self.iteration, self.call, self.entry = iteration, call, entry
        self.it, self.k, self.dropped = -1, 0, 0

    def begin(self, it):
        self.it, self.k = it, 0

    def __call__(self, a, b):
        k, self.k = self.k, self.k + 1
        if self.it == self.iteration and k == self.call:
            a = a.clone()
            a[self.entry] = 0.0
            self.dropped += 1
        return torch.dot(a, b)


# ---- the layout of the element kernels
LB_THREADS, LB_MAX_G = 256, 1024


class DeviceOrderDot:
    """The summation tree of csrc/lbfgs.hip restated, so that the statement can be asked for the device's BITS: workgroup
    g owns entries [g chunk, (g + 1) chunk); thread t adds its rounded products t, t + 256, ... in that order; lb_block_sum
    halves the 256 sums (t += t + w for w = 128 .. 1); lb_finish does the same with the G partials.  The zeros that pad a
    short row add exactly."""

    def __init__(self, n):
        self.n = int(n)
        self.G, self.chunk = layout(self.n)

    @staticmethod
    def _block_sum(rows):
        """rows f64 [R, m] -> [R]: one workgroup per row."""
        R, m = rows.shape
        passes = (m + LB_THREADS - 1) // LB_THREADS
        x = torch.zeros(R, passes * LB_THREADS, dtype=torch.float64)
        x[:, :m] = rows
        x = x.reshape(R, passes, LB_THREADS)
        acc = x[:, 0].clone()
        for p in range(1, passes):
            acc = acc + x[:, p]
        w = LB_THREADS // 2
        while w:
            acc = acc[:, :w] + acc[:, w:2 * w]
            w //= 2
        return acc[:, 0]

    def __call__(self, a, b):
        prod = torch.zeros(self.G * self.chunk, dtype=torch.float64)
        prod[:self.n] = a * b
        return self._block_sum(self._block_sum(prod.reshape(self.G, self.chunk)).reshape(1, self.G))[0]


def layout(n):
    """(G, chunk) of a handle with n = 3N entries.  Restates the two lines of adf_lbfgs_create (csrc/lbfgs.hip) that follow
    "about 4 entries per thread, at most LB_MAX_G workgroups":
        g = (n + 4 * LB_THREADS - 1) / (4 * LB_THREADS);  G = clamp(g, 1, LB_MAX_G);  chunk = (n + G - 1) / G
    A change of LB_THREADS or LB_MAX_G there moves every seam: CASES below has to be worked out again."""
    g = (n + 4 * LB_THREADS - 1) // (4 * LB_THREADS)
    G = max(1, min(LB_MAX_G, g))
    return G, (n + G - 1) // G


# ---- the case table: the smallest sizes on either side of each seam.  Every listed case has a 1-atom system, a system
# whose 7 atoms are all fixed and, where the atom count allows it (from three_wg on), a system of 600 atoms, so that the
# one-workgroup-per-system kernels stride more than twice; one_wg / two_wg hold 341 / 342 atoms in all and their largest
# system has 300 (two passes over the atoms, four over the entries).  Amplitude (distance from the minimum) and stiffness
# are staggered: the 300 / 600 atom system stays far from its minimum, the 1-atom system's mask clears at iteration 2, the
# 40 000 / 150 000 atom system's at iteration 3, and the last system of the three large cases keeps moving, so the last
# partials are never zero.
#   one_wg      n = 1023       (1, 1023)     last size with one workgroup; 4 passes per thread, the last one partial
#   two_wg      n = 1026       (2, 513)      lb_finish over more than one partial; the seam (entry 513 = atom 171) lies inside
#                                            the 300-atom system.  513 = 3 x 171, so no atom is split here; from three_wg on one is
#   three_wg    n = 2100       (3, 700)      uneven passes (700 = 2 x 256 + 188); atoms 233 and 466 split across workgroups
#   finish_256  n = 262 143    (256, 1024)   lb_finish: every thread holds exactly one partial
#   finish_257  n = 262 146    (257, 1021)   lb_finish takes a second pass for one thread
#   cap         n = 1 048 800  (1024, 1025)  G capped at LB_MAX_G, chunk above 4 x 256; the last workgroup holds 225 entries
#   many_systems  300 systems of 1 - 4 atoms: B > 256, the strided loops over sys_absmax / mask; only system 299 is far from
#               its minimum, every other one is converged or within a few 1e-3 A of it (system 99: 2e-5 A, see MUTATE)
Case = namedtuple("Case", "natoms layout amp k fmax fixed_sys")
_MANY = [2] + [(i % 4) + 1 for i in range(1, 300)]   # 751 atoms, (3, 751): both workgroup seams fall inside a system
CASES = {
    "one_wg": Case([1, 7, 300, 33], (1, 1023), [0.07, 0.5, 1.0, 0.01], [3.0, 4.0, 5.0, 7.0], 0.13, 1),
    "two_wg": Case([300, 1, 7, 34], (2, 513), [1.0, 0.07, 0.5, 0.01], [5.0, 3.0, 4.0, 7.0], 0.13, 2),
    "three_wg": Case([1, 600, 7, 92], (3, 700), [0.07, 1.0, 0.5, 0.01], [3.0, 5.0, 4.0, 7.0], 0.13, 2),
    "finish_256": Case([1, 600, 7, 40000, 46773], (256, 1024), [0.07, 1.0, 0.5, 0.08, 1.0], [3.0, 5.0, 4.0, 2.0, 6.0], 0.13, 2),
    "finish_257": Case([1, 600, 7, 40000, 46774], (257, 1021), [0.07, 1.0, 0.5, 0.08, 1.0], [3.0, 5.0, 4.0, 2.0, 6.0], 0.13, 2),
    "cap": Case([1, 600, 7, 150000, 198992], (1024, 1025), [0.07, 1.0, 0.5, 0.08, 1.0], [3.0, 5.0, 4.0, 2.0, 6.0], 0.13, 2),
    "many_systems": Case(_MANY, layout(3 * sum(_MANY)), [2e-5 if i == 99 else 1e-3 * (1 + i % 5) for i in range(299)] + [1.0],
                         [2.0 + (i % 8) for i in range(299)] + [5.0], 0.02, 150),
}
BIG = ("finish_256", "finish_257", "cap")       # one (memory, early_stop_batch) combination each
ITERATIONS = {name: 8 if name == "cap" else 12 for name in CASES}


def combos(name):
    """The (memory, early_stop_batch) combinations a case runs with (cap: memory 2, 8 iterations)."""
    if name == "cap":
        return [(2, False)]
    if name in BIG:
        return [(3, False)]
    return [(1, False), (1, True), (3, False), (3, True)]


# The chunk whose last entry DroppingDot loses.  The entry has to matter little enough for the f32 positions not to see
# it: a typical entry of a thousand would move alpha by 1e-3.  The cases of a thousand entries lose the last entry of the
# last chunk, in the small-amplitude last system; the large cases lose the last entry of chunk 50, in the 40 000 / 150 000
# atom system (one entry of 1e5 - 1e6); many_systems loses the last entry of chunk 0, in system 99.
MUTATE = {"one_wg": 0, "two_wg": 1, "three_wg": 2, "finish_256": 50, "finish_257": 50, "cap": 50, "many_systems": 0}


def mutate_entry(name):
    n = 3 * sum(CASES[name].natoms)
    _, chunk = layout(n)
    return min((MUTATE[name] + 1) * chunk, n) - 1


# ---- scripts: the forces of a run are the harmonic ones times a gain per iteration (a number, or one per atom)
SKIP_GAINS = (1.0, 1.0, 1e-9, 1.0, 1.0)


def script_gains(inp, script):
    """None (gain 1 throughout), "skip" (SKIP_GAINS: iteration 2 is skipped) or "only_299" (SKIP_GAINS, but system 299
    keeps gain 1 at iteration 2: the step is not skipped)."""
    if script is None:
        return None
    gains = list(SKIP_GAINS)
    if script == "only_299":
        gains[2] = torch.full((len(inp.batch),), SKIP_GAINS[2])
        gains[2][inp.batch == 299] = 1.0
    return gains


SKIP_RUNS = (("two_wg", "skip"), ("many_systems", "skip"), ("many_systems", "only_299"))     # memory 3, 5 iterations


def runs(name):
    """(memory, early_stop_batch, iterations) of every trajectory run of a case."""
    out = [(m, e, ITERATIONS[name]) for m, e in combos(name)]
    return out + ([(50, False, 6)] if name == "three_wg" else [])   # memory 50: the history is never full


# Largest max |z_a - z_b| / max |z_a| between the statement with torch.dot and with ShuffledDot (SHUFFLE_SEEDS) over the
# iterations and combinations of a case, and of each skip script ("case:script"; an iteration whose forces are 1e-9 of the
# history's is worse conditioned, so these have numbers of their own).  tests/test_relax_coupled_host.py measures them again
# and asserts the stored ones are not below.  The device's order is a third order of the same sums: its z may differ from
# the statement's by Z_MARGIN x the spread of the same run.
Z_SPREAD = {
    "one_wg": 6e-16, "two_wg": 4e-16, "three_wg": 7e-16, "finish_256": 5e-14, "finish_257": 4e-14, "cap": 4e-14,
    "many_systems": 2.5e-15, "two_wg:skip": 2.5e-14, "many_systems:skip": 5e-15, "many_systems:only_299": 4e-15,
}
SHUFFLE_SEEDS = (7, 8, 9)
Z_MARGIN = 16.0
Z_TOL_CAP = 1e-9      # a condition, not a measurement: no case may need more


def z_tol(name):
    return Z_MARGIN * Z_SPREAD[name]


def z_err(z, z_ref):
    """max |z - z_ref| / max |z_ref| (nan when either holds a NaN)."""
    z, z_ref = torch.as_tensor(z).cpu().double().reshape(-1), torch.as_tensor(z_ref).cpu().double().reshape(-1)
    return float((z - z_ref).abs().max() / z_ref.abs().max())


# ---- scripted inputs
Inputs = namedtuple("Inputs", "natoms batch pos xstar k_atom fixed fmax")


def make_inputs(name, natoms=None):
    """Positions in [4, 8) A (one f32 ulp = 4.8e-7 A everywhere, far above the ulp of a 0.04 A step), minima x* within the
    system's amplitude of them, per-system stiffness; the atoms of the case's fixed system are fixed."""
    c = CASES[name]
    natoms = list(c.natoms if natoms is None else natoms)
    n_atoms = sum(natoms)
    g = torch.Generator().manual_seed(1000 + n_atoms)
    batch = torch.repeat_interleave(torch.arange(len(natoms)), torch.tensor(natoms))
    pos = (4.0 + 4.0 * torch.rand(n_atoms, 3, generator=g)).float()
    amp = torch.tensor(c.amp[:len(natoms)], dtype=torch.float32)[batch].unsqueeze(1)
    offset = 2.0 * torch.rand(n_atoms, 3, generator=g) - 1.0
    if len(natoms) < 10 and 1 in natoms:      # the 1-atom system sits exactly its amplitude from its minimum: its mask clears on schedule
        offset[batch == natoms.index(1)] = torch.tensor([0.6, -0.64, 0.48])
    xstar = (pos + amp * offset).float()
    k_atom = torch.tensor(c.k[:len(natoms)], dtype=torch.float32)[batch].unsqueeze(1)
    fixed = (batch == c.fixed_sys) if len(natoms) > 1 else torch.zeros(n_atoms, dtype=torch.bool)
    return Inputs(natoms, batch, pos, xstar, k_atom, fixed, c.fmax)


def harmonic_forces(pos, inp, gain=None):
    """f = -(k_s (x - x*)) in f32 on pos's device, times an optional per-atom gain; fixed atoms get zero."""
    dev = pos.device
    f = -(inp.k_atom.to(dev) * (pos - inp.xstar.to(dev)))
    if gain is not None:
        f = f * torch.as_tensor(gain, dtype=torch.float32, device=dev).reshape(-1, 1)
    return f.masked_fill(inp.fixed.to(dev).reshape(-1, 1), 0.0)


def system_masks(forces, inp):
    """(max |f_atom| of every system in f64, the update mask max >= fmax) as check_convergence states them."""
    mf = torch.stack([max_force(f) for f in split_systems(forces.detach().cpu(), inp.natoms)])
    return mf, mf.ge(inp.fmax)
