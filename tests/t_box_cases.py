"""What the tests of the Student-t box entries share (mlmc_copula_box_prob_t_batch / _draws_t_batch, include/mlmc_hip.h; Genz and
Bretz's mixing variable): tests/test_t_box_cpu.py, tests/test_gpu_t_box.py, tests/test_gpu_t_box_api.py.  Nothing here touches the
device.

  mp_t_score   the t score of a normal score in mpmath (MP_DIGITS digits): the root of the regularised incomplete beta function;
  t_twin       the chain of the header in NumPy, vectorised over the points: tests/box_prob_cases.twin with lo / s, hi / s in the
               place of the limits (tests/test_t_box_cpu.py holds the two against each other bit for bit, point by point);
  mixing_points, problem, SHAPES   the coordinates and the small problems of the GPU tests.
"""
import mpmath
import numpy as np
from scipy import special

from tests import box_prob_cases as bc

MP_DIGITS = 40
DOFS = (1.0, 3.0, 7.5, 64.0)
# probability levels of the limit mapping, 1e-12 .. 1 - 1e-12; the normal scores of these are the inputs
_LOW = (1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 0.01, 0.05, 0.1, 0.25, 0.4)
LEVELS = np.array(_LOW + (0.5,) + tuple(1.0 - p for p in reversed(_LOW)))

# The largest error of `simple_distribution.t_scores` (SciPy's ndtr followed by stdtrit) against mp_t_score over LEVELS x DOFS, in
# ulps of the score, as tests/test_t_box_cpu.py measures it (it prints the figure per nu); the gate is twice this record.  SciPy
# 1.15's stdtrit stops its iteration at about 2e-11 relative: 1.42e5 (nu = 1), 1.09e5 (3), 6.7e4 (7.5), 1.54e5 (64) ulps, at levels
# between 0.01 and 0.25; most levels take a few ulps.  A limit that is off by 3e-11 relative moves a box probability by less than
# that times its logarithmic derivative, far below the integration error of any n in use.
T_SCORE_ULPS_OBSERVED = 1.54e5
T_SCORE_ULPS_GATE = 2.0 * T_SCORE_ULPS_OBSERVED


def _mp_t_lower(nu, y):
    """T_nu(y) for y <= 0 in the working precision: I_x(nu / 2, 1 / 2) / 2 at x = nu / (nu + y^2)"""
    return mpmath.betainc(nu / 2, mpmath.mpf(1) / 2, 0, nu / (nu + y * y), regularized=True) / 2


def mp_t_score(dof, zn):
    """y with T_dof(y) = Phi(zn) for the double zn, as an mpf: the root of the regularised incomplete beta function in the lower
    tail (for zn > 0 by the symmetry of both laws), found on the logarithm so that a deep tail converges like the centre"""
    zn = float(zn)
    if zn == 0.0:
        return mpmath.mpf(0)
    with mpmath.workdps(MP_DIGITS):
        nu = mpmath.mpf(float(dof))
        logp = mpmath.log(mpmath.ncdf(-abs(mpmath.mpf(zn))))
        start = float(special.stdtrit(float(dof), special.ndtr(-abs(zn))))
        y = mpmath.findroot(lambda t: mpmath.log(_mp_t_lower(nu, t)) - logp, (mpmath.mpf(start) * (1 + mpmath.mpf(2) ** -40), mpmath.mpf(start)),
                            solver="secant", tol=mpmath.mpf(10) ** -(MP_DIGITS - 8), maxsteps=60)
        return -y if zn > 0 else +y


def score_ulps(y, ref):
    """|y - ref| in ulps of the double nearest to ref (0 where both are 0)"""
    with mpmath.workdps(MP_DIGITS):
        r = float(ref)
        if r == 0.0:
            return 0.0 if y == 0.0 else np.inf
        return float(abs(mpmath.mpf(float(y)) - ref) / mpmath.mpf(float(np.spacing(abs(r)))))


def t_twin(L, lo, hi, s, w):
    """f [n] of one box under the t law: the chain of tests/box_prob_cases.twin on the limits lo / s, hi / s of every point (s [n] the
    mixing scales, w [M - 1, n] the chain's coordinates), every operation the one of the header"""
    L = np.asarray(L, dtype=np.float64)
    M, n = L.shape[0], s.size
    f = np.ones(n)
    y = np.zeros((max(M - 1, 0), n))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(M):
            lt, ht = lo[i] / s, hi[i] / s
            acc = np.zeros(n)
            for k in range(i):
                acc = acc + L[i, k] * y[k]
            a, b = (lt - acc) / L[i, i], (ht - acc) / L[i, i]
            refl = a > 0.0
            d, e = special.ndtr(np.where(refl, -b, a)), special.ndtr(np.where(refl, -a, b))
            width = np.where(lt < ht, e - d, 0.0)
            f = f * width
            if i < M - 1:
                yy = special.ndtri(np.minimum(np.maximum(d + w[i] * width, bc.P_LO), bc.P_HI))
                y[i] = np.where(refl, -yy, yy)
    return f


# ---- the GPU tests' problems ------------------------------------------------------------------------------------------------------
MIX = 0                                                # the default mixing stream; chain coordinate i then takes stream i + 1
# (M, n, first, qmc): Philox with first = 37 (ragged first and last blocks), Sobol' from 0; M = 128 once at n = 64
SHAPES = ((1, 27, 37, False), (2, 1, 37, False), (2, 200, 37, False), (3, 64, 37, False), (12, 27, 37, False),
          (1, 64, 0, True), (3, 256, 0, True), (12, 64, 0, True), (128, 64, 0, True))


def chain_streams(M, draws=False):
    return list(range(1, (M if draws else M - 1) + 1))


def mixing_points(seed, first, n, qmc, stream=MIX):
    """p0 [n]: the mixing coordinate of the points first .. first + n - 1 under `seed`"""
    return bc.points(seed, [stream], first, n, qmc)[0]


def problem(M, B, seed=0):
    """(L [M, M], lo [B, M], hi [B, M]) in t-score space: the boxes of tests/box_prob_cases.boxes; box 1 (B > 1) has infinite upper
    limits, and the last box of B = 4 gets an EMPTY component (lo > hi in its last component: probability exactly 0)"""
    L = bc.chol_factor(M, 300 + M + seed)
    lo, hi = bc.boxes(M, B, 400 + M + seed)
    if B == 4:
        lo[3, M - 1], hi[3, M - 1] = 0.5, -0.5
    return L, lo, hi
