"""Locating a lead's viewing angle by a scored panorama search (Model_nefnet.locate, engine.locate, Solver.locate; definitions:
include/nefnet_hip.h, nef_locate_score_args): the level-0 grid, the checks of the search's settings and their config keys.

Level 0 is a regular grid shared by all samples: theta1_i = lo1 + i * d1 (i < n1), theta2_k = lo2 + k * d2 (k < n2), candidate index
i * n2 + k, d = (hi - lo) / max(n - 1, 1); n == 1 pins an axis at `lo` with step 0.  Levels 1 .. `levels` lay (2 radius + 1)^2
candidates around each pair's running best, the step halving at every level (s_j = s_(j-1) / 2, s_0 = d), in fp32."""
import math
from typing import NamedTuple, Optional

import numpy as np

SCORES = ("mse", "corr")
MAX_RADIUS = 16      # nef_locate_cands


class Grid(NamedTuple):
    """n1 x n2 angles over [lo1, hi1] x [lo2, hi2] (radians)."""
    n1: int = 9
    n2: int = 19
    lo1: float = math.pi / 3
    hi1: float = math.pi
    lo2: float = -math.pi / 2
    hi2: float = math.pi / 2

    @property
    def size(self):
        return self.n1 * self.n2

    @property
    def steps(self):
        """(d1, d2): 0 for a pinned axis."""
        return ((self.hi1 - self.lo1) / max(self.n1 - 1, 1) if self.n1 > 1 else 0.0,
                (self.hi2 - self.lo2) / max(self.n2 - 1, 1) if self.n2 > 1 else 0.0)

    def index(self, i, k):
        return i * self.n2 + k

    def thetas(self):
        """fp32 [n1 * n2, 2], candidate i * n2 + k = (lo1 + i * d1, lo2 + k * d2), formed in fp64 and rounded once."""
        d1, d2 = self.steps
        t1 = self.lo1 + np.arange(self.n1, dtype=np.float64) * d1
        t2 = self.lo2 + np.arange(self.n2, dtype=np.float64) * d2
        out = np.empty((self.n1, self.n2, 2), dtype=np.float64)
        out[..., 0] = t1[:, None]
        out[..., 1] = t2[None, :]
        return out.reshape(-1, 2).astype(np.float32)

    def check(self):
        for name, n in (("n1", self.n1), ("n2", self.n2)):
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
                raise ValueError(f"locate grid: {name} must be an integer >= 1, got {n!r}")
        for name, lo, hi, n in (("theta1", self.lo1, self.hi1, self.n1), ("theta2", self.lo2, self.hi2, self.n2)):
            if not (isinstance(lo, (int, float)) and isinstance(hi, (int, float)) and math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"locate grid: the {name} range must be two finite numbers, got {lo!r}, {hi!r}")
            if hi < lo or (n > 1 and not hi > lo):
                raise ValueError(f"locate grid: the {name} range [{lo}, {hi}] is empty for {n} points")
        if self.size > (1 << 20):
            raise ValueError(f"locate grid: {self.n1} x {self.n2} candidates is more than 2^20")
        return self


def as_grid(grid):
    """None (the default 9 x 19 grid over LEAD_THETA's span), a Grid, or (n1, n2) over the default range."""
    if grid is None:
        return Grid()
    if isinstance(grid, Grid):
        return grid.check()
    try:
        n1, n2 = grid
    except (TypeError, ValueError):
        raise ValueError(f"locate grid: expected a Grid or (n1, n2), got {grid!r}") from None
    return Grid(n1, n2).check()


class Settings(NamedTuple):
    grid: Grid
    score: str
    levels: int
    radius: int


def check_settings(grid=None, score="corr", levels=3, radius=2, eps=None):
    """ValueError for a bad grid, score name, level count, radius or eps; the checked Settings otherwise."""
    g = as_grid(grid)
    if score not in SCORES:
        raise ValueError(f"locate score must be one of {SCORES}, got {score!r}")
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= levels <= 24:
        raise ValueError(f"locate levels must be an integer in 0 .. 24 (fp32 steps halve every level), got {levels!r}")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"locate radius must be an integer in 0 .. {MAX_RADIUS}, got {radius!r}")
    if levels > 0 and radius < 1:
        raise ValueError("locate radius must be >= 1 when levels > 0 (a radius of 0 only re-scores the best)")
    if eps is not None and not (isinstance(eps, (int, float)) and not isinstance(eps, bool) and math.isfinite(eps) and eps > 0):
        raise ValueError(f"locate eps must be a finite number > 0, got {eps!r}")
    return Settings(g, score, int(levels), int(radius))


def from_cfg(cfg, force=False) -> Optional[dict]:
    """The keyword arguments of Model_nefnet.locate from SOLVER.locate_* (checked), or None with SOLVER.locate_eval off -- then the
    other keys are not looked at.  force: the settings whether or not the key is on (Solver.locate called by hand)."""
    s = cfg.SOLVER
    if not force and not bool(s.get("locate_eval", False)):
        return None
    n = s.get("locate_grid", [9, 19])
    rng = s.get("locate_range_deg", [[60, 180], [-90, 90]])
    try:
        (n1, n2), ((lo1, hi1), (lo2, hi2)) = n, rng
        grid = Grid(n1, n2, math.radians(lo1), math.radians(hi1), math.radians(lo2), math.radians(hi2))
    except (TypeError, ValueError):
        raise ValueError(f"SOLVER.locate_grid {n!r} / SOLVER.locate_range_deg {rng!r}: expected [n1, n2] and [[lo1, hi1], [lo2, hi2]]") from None
    eps = s.get("corr_eps", 1e-8)
    st = check_settings(grid, s.get("locate_score", "corr"), s.get("locate_levels", 3), s.get("locate_radius", 2), eps)
    return dict(grid=st.grid, score=st.score, levels=st.levels, radius=st.radius, eps=float(eps))


def level_steps(grid, levels):
    """[(s1, s2)] of levels 1 .. levels as fp32: the grid's steps rounded to fp32, halved (exactly) once per level."""
    d1, d2 = (np.float32(d) for d in grid.steps)
    out = []
    for _ in range(levels):
        d1, d2 = np.float32(d1 * np.float32(0.5)), np.float32(d2 * np.float32(0.5))
        out.append((d1, d2))
    return out


class LocateResult(NamedTuple):
    """theta fp32 [B, R, 2], score fp64 [B, R], index int64 [B, R] (the level-0 candidate index, -1 without a finite score), theta0 /
    score0: the level-0 best; scores fp64 [B, R, A] (return_scores) and trace (return_trace): one dict per level 1 .. levels with
    `cands` [B, R * G, 2], `scores` [B, R, G], `theta`, `score` after the level.  The R dimension is squeezed for a 2-D `observed`."""
    theta: object
    score: object
    index: object
    theta0: object
    score0: object
    scores: object = None
    trace: object = None
