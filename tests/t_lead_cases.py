"""What the tests of the t box entries with a conditioned lead component share (mlmc_copula_box_prob_tl_batch / _draws_tl_batch,
include/mlmc_hip.h): tests/test_t_lead_cpu.py, tests/test_gpu_t_lead.py, tests/test_gpu_t_lead_api.py.  Nothing
here touches the device.

  lead_twin          steps 1 - 7 of the header in NumPy, vectorised over the points, with SciPy for T, T^-1 and chi2;
  plain_twin_orthant the plain mixing of the _t_batch entries on the same kind of problem (what the conditioned lead replaces);
  independent_reference / equicorrelated_reference   the functions that made the tabulated references below;
  INDEPENDENT, EQUI  the tabulated references;  TWIN  what the twin gives on the points of the GPU tests (recorded on the CPU).
"""
import mpmath
import numpy as np
from scipy import integrate, special

from tests import box_prob_cases as bc

MP_DIGITS = 40
DOFS = (1.0, 3.0, 7.5, 64.0)
LEVELS = (1e-3, 1e-6, 1e-9, 1e-12)
V_CAP = 2.0 ** 500
MIX = 0                                                # the default mixing stream; coordinate i (the lead: 0) takes stream i + 1
CLOSED_N, CLOSED_SEEDS = 4096, tuple(range(8))


def conditional_scale(p0, dof_mix):
    """sqrt(nu / chi2_nu quantile of p0): what mlmc_chi2_conditional_scale computes"""
    a = 0.5 * float(dof_mix)
    return np.sqrt(a / special.gammaincinv(a, p0))


def lead_weights(L, lo, hi, dof):
    """(a, bq, refl, d, e, W0) of step 2 for one box"""
    with np.errstate(divide="ignore"):
        a, bq = np.float64(lo[0]) / L[0, 0], np.float64(hi[0]) / L[0, 0]
    refl = a > 0.0
    d, e = special.stdtr(dof, -bq if refl else a), special.stdtr(dof, -a if refl else bq)
    return a, bq, refl, d, e, (e - d if a < bq else 0.0)


def lead_scores(L, lo, hi, dof, w0):
    """(v [n], W0) of steps 2 and 3 for one box on the lead's uniforms w0 [n]"""
    a, bq, refl, d, _, W0 = lead_weights(L, lo, hi, dof)
    p = np.minimum(np.maximum(d + w0 * W0, bc.P_LO), bc.P_HI)
    v = special.stdtrit(dof, p)
    v = -v if refl else v
    v = np.minimum(np.maximum(v, a), bq)
    return np.minimum(np.maximum(v, -V_CAP), V_CAP), W0


def lead_twin(L, lo, hi, dof, p0, w, draws=False):
    """(f [n], v [n], sc [n]) of one box: p0 [n] the mixing uniforms, w [>= M - 1, n] the coordinates (w[0] the lead's, w[i] the one
    of component i); with draws also z [M, n], the stored t scores (w has M rows then)"""
    L = np.asarray(L, dtype=np.float64)
    M, n = L.shape[0], p0.size
    g0 = conditional_scale(p0, dof + 1.0)
    v, W0 = lead_scores(L, lo, hi, dof, w[0])
    sc = g0 * np.sqrt((dof + v * v) / (dof + 1.0))
    y = np.zeros((M, n))
    y[0] = v / sc
    g = np.ones(n)
    z = np.zeros((M, n))
    z[0] = np.minimum(np.maximum(v * L[0, 0], lo[0]), hi[0])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(1, M):
            lt, ht = lo[i] / sc, hi[i] / sc
            acc = np.zeros(n)
            for k in range(i):
                acc = acc + L[i, k] * y[k]
            a, b = (lt - acc) / L[i, i], (ht - acc) / L[i, i]
            refl = a > 0.0
            d, e = special.ndtr(np.where(refl, -b, a)), special.ndtr(np.where(refl, -a, b))
            width = np.where(lt < ht, e - d, 0.0)
            g = g * width
            if draws or i < M - 1:
                yy = special.ndtri(np.minimum(np.maximum(d + w[i] * width, bc.P_LO), bc.P_HI))
                y[i] = np.where(refl, -yy, yy)
                zn = np.minimum(np.maximum(acc + L[i, i] * y[i], lt), ht)
                z[i] = np.minimum(np.maximum(zn * sc, lo[i]), hi[i])
    f = W0 * g
    return (f, v, sc, z) if draws else (f, v, sc)


def points_of(seed, M, first, n, qmc, draws=False):
    """(p0 [n], w [M - 1 or M, n]) under the default streams: mixing stream 0, coordinate i stream i + 1"""
    count = M if draws else max(M - 1, 1)
    pts = bc.points(seed, [MIX] + list(range(1, count + 1)), first, n, qmc)
    return pts[0], pts[1:]


def twin_replicates(L, lo, hi, dof, seeds, n, first=0, qmc=True):
    """the twin's mean per seed [R] for one box, and the integrand [R, n]"""
    M = np.asarray(L).shape[0]
    f = np.array([lead_twin(L, lo, hi, dof, *points_of(s, M, first, n, qmc))[0] for s in seeds])
    return f.mean(axis=1), f


def plain_twin_orthant(L, lo, hi, dof, seeds, n, first=0, qmc=True):
    """the mean per seed [R] under PLAIN mixing (tests/t_box_cases.t_twin on the default streams of the _t_batch entries)"""
    from tests import t_box_cases as tb
    M = np.asarray(L).shape[0]
    out = []
    for s in seeds:
        pts = bc.points(s, [MIX] + list(range(1, M)), first, n, qmc)
        out.append(tb.t_twin(L, lo, hi, np.sqrt(0.5 * dof / special.gammaincinv(0.5 * dof, pts[0])), pts[1:]).mean())
    return np.array(out)


def ess_fraction(weights):
    """(sum w)^2 / (n sum w^2) over the last axis"""
    w = np.asarray(weights, dtype=np.float64)
    return np.sum(w, axis=-1) ** 2 / (w.shape[-1] * np.sum(w * w, axis=-1))


def t_upper_quantile(dof, q):
    """t with P(T_dof > t) = q, through the lower tail"""
    return -float(special.stdtrit(dof, q))


# ---- references -------------------------------------------------------------------------------------------------------------------
def independent_reference(M, dof, lo, hi):
    """P(lo < Y_i < hi for all i) for the factor I: Y = z / sqrt(W), W = chi2_nu / nu, the 1-D integral
    E_W[prod_i (Phi(hi_i sqrt(W)) - Phi(lo_i sqrt(W)))] by mpmath at MP_DIGITS digits.  The variable is x = W t^2 with t the smallest
    finite |limit|, so that the integrand lives on x = O(1) at any depth of the box."""
    with mpmath.workdps(MP_DIGITS):
        nu = mpmath.mpf(float(dof))
        lo = [mpmath.mpf(float(x)) for x in np.broadcast_to(lo, (M,))]
        hi = [mpmath.mpf(float(x)) for x in np.broadcast_to(hi, (M,))]
        t = min([abs(x) for x in lo + hi if mpmath.isfinite(x) and x != 0] or [mpmath.mpf(1)])
        a = nu / 2
        logc = a * mpmath.log(a) - mpmath.loggamma(a)

        def integrand(x):
            if x == 0:
                return mpmath.mpf(0)
            W = x / (t * t)
            r = mpmath.sqrt(W)
            prod = mpmath.mpf(1)
            for l, h in zip(lo, hi):
                # through the lower tail on either side
                if l > 0:
                    prod *= mpmath.ncdf(-l * r) - (mpmath.ncdf(-h * r) if mpmath.isfinite(h) else 0)
                else:
                    prod *= (mpmath.ncdf(h * r) if mpmath.isfinite(h) else 1) - (mpmath.ncdf(l * r) if mpmath.isfinite(l) else 0)
            return prod * mpmath.exp(logc + (a - 1) * mpmath.log(W) - a * W) / (t * t)
        cuts = [mpmath.mpf(0)] + [mpmath.mpf(2) ** k for k in range(-40, 41, 4)] + [mpmath.inf]
        return mpmath.quad(integrand, cuts)


def equicorrelated_reference(M, dof, t):
    """P(Y_i > t for all i) under equicorrelation 1/2: Y_i = (z_0 + e_i) / sqrt(2 W), the 2-D one-factor integral
    E_W E_z0[Phi(z_0 - t sqrt(2 W))^M] by nested SciPy quadrature (x = W t^2 as above)"""
    a = 0.5 * dof
    logc = a * np.log(a) - special.gammaln(a)

    def inner(x):
        c = np.sqrt(2.0 * x)
        return integrate.quad(lambda z: np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) * special.ndtr(z - c) ** M, -12.0, 12.0 + c,
                              epsabs=0, epsrel=1e-12, limit=400)[0]

    def outer(x):
        W = x / (t * t)
        return inner(x) * np.exp(logc + (a - 1) * np.log(W) - a * W) / (t * t)
    cuts = [0.0] + [2.0 ** k for k in range(-40, 13, 2)]
    return sum(integrate.quad(outer, lo, hi, epsabs=0, epsrel=1e-11, limit=200)[0] for lo, hi in zip(cuts[:-1], cuts[1:]))


TWO_SIDED = (-0.5, 1.5)                                # the one two-sided box: every component in (-0.5, 1.5)


def make_tables():
    """the tables below, as they were made"""
    ind = {}
    for M in (2, 12):
        for dof in DOFS:
            for q in LEVELS:
                ind[(M, dof, q)] = float(independent_reference(M, dof, t_upper_quantile(dof, q), np.inf))
            ind[(M, dof, "box")] = float(independent_reference(M, dof, TWO_SIDED[0], TWO_SIDED[1]))
    equi = {(M, 3.0, q): equicorrelated_reference(M, 3.0, t_upper_quantile(3.0, q)) for M in (2, 3) for q in LEVELS}
    return ind, equi


# (M, nu, level or "box") -> probability; upper orthants beyond the t quantile of level 1 - q (t_upper_quantile), factor I
INDEPENDENT = {
    (2, 1.0, 0.001): 0.0002928938003864812,
    (2, 1.0, 1e-06): 2.9289321881399315e-07,
    (2, 1.0, 1e-09): 2.9289321881345246e-10,
    (2, 1.0, 1e-12): 2.928932188134526e-13,
    (2, 1.0, 'box'): 0.27511365492362105,
    (2, 3.0, 0.001): 0.00011838311736482892,
    (2, 3.0, 1e-06): 1.1613888619446618e-07,
    (2, 3.0, 1e-09): 1.1611674711346648e-10,
    (2, 3.0, 1e-12): 1.1611652575279356e-13,
    (2, 3.0, 'box'): 0.3376461750526054,
    (2, 7.5, 0.001): 3.0400166877564363e-05,
    (2, 7.5, 1e-06): 1.968366085248017e-08,
    (2, 7.5, 1e-09): 1.8436237027926615e-11,
    (2, 7.5, 1e-12): 1.824741569173051e-14,
    (2, 7.5, 'box'): 0.36633512877370084,
    (2, 64.0, 0.001): 2.105965838213723e-06,
    (2, 64.0, 1e-06): 2.5710234064946406e-11,
    (2, 64.0, 1e-09): 1.0554330844912939e-15,
    (2, 64.0, 1e-12): 9.829785798758778e-20,
    (2, 64.0, 'box'): 0.3871475955303169,
    (12, 1.0, 0.001): 5.946032628113629e-08,
    (12, 1.0, 1e-06): 5.946013530130018e-11,
    (12, 1.0, 1e-09): 5.94601353011175e-14,
    (12, 1.0, 1e-12): 5.946013530111752e-17,
    (12, 1.0, 'box'): 0.019588618316937718,
    (12, 3.0, 0.001): 1.4565657242048629e-09,
    (12, 3.0, 1e-06): 1.4098522346831269e-12,
    (12, 3.0, 1e-09): 1.4093968022252504e-15,
    (12, 3.0, 1e-12): 1.4093922490465602e-18,
    (12, 3.0, 'box'): 0.010528629842936099,
    (12, 7.5, 0.001): 2.0996354658712064e-12,
    (12, 7.5, 1e-06): 9.252490925192294e-16,
    (12, 7.5, 1e-09): 8.235371789673759e-19,
    (12, 7.5, 1e-12): 8.087137092668185e-22,
    (12, 7.5, 'box'): 0.00667687873434139,
    (12, 64.0, 0.001): 1.216235198159309e-24,
    (12, 64.0, 1e-06): 2.95713583736955e-35,
    (12, 64.0, 1e-09): 1.9396665929940392e-42,
    (12, 64.0, 1e-12): 4.20469824998838e-48,
    (12, 64.0, 'box'): 0.003936409264612935,
}
# (M, 3.0, level) -> probability of the upper orthant under equicorrelation 1/2
EQUI = {
    (2, 3.0, 0.001): 0.00031608341076129264,
    (2, 3.0, 1e-06): 3.1253557656994625e-07,
    (2, 3.0, 1e-09): 3.125003557397341e-10,
    (2, 3.0, 1e-12): 3.125000035574339e-13,
    (3, 3.0, 0.001): 0.0001628958321157518,
    (3, 3.0, 1e-06): 1.6041249486332019e-07,
    (3, 3.0, 1e-09): 1.6038792629147123e-10,
    (3, 3.0, 1e-12): 1.603876806322051e-13,
}
# (kind, M, nu, level) -> (prob, relative stderr) of `twin_replicates` on the points of the GPU tests (CLOSED_N Sobol' points, CLOSED_SEEDS,
# default streams), recorded on the CPU.  The deep orthants of M = 12 independent components at nu >= 7.5 are NOT resolved by the lead
# alone (relative stderr 0.2 .. 1): eleven more components want a large scale there, which only conditioning beyond the lead would give.
TWIN = {
    ('I', 2, 1.0, 0.001): (0.0002928934263294993, 4.550001529518887e-06),
    ('I', 2, 1.0, 1e-06): (2.9289284476587117e-07, 4.5500138968711735e-06),
    ('I', 2, 1.0, 1e-09): (2.928928447653354e-10, 4.550013896870879e-06),
    ('I', 2, 1.0, 1e-12): (2.9289284476533553e-13, 4.55001389688623e-06),
    ('I', 2, 1.0, 'box'): (0.27511387508537116, 2.0294056556579297e-06),
    ('I', 2, 3.0, 0.001): (0.00011838647927894302, 3.266477010192856e-05),
    ('I', 2, 3.0, 1e-06): (1.1614227226473791e-07, 3.362194809071898e-05),
    ('I', 2, 3.0, 1e-09): (1.1612013341997573e-10, 3.363161541069552e-05),
    ('I', 2, 3.0, 1e-12): (1.1611991206170996e-13, 3.3631712087186434e-05),
    ('I', 2, 3.0, 'box'): (0.33764570822154527, 4.449487188754057e-06),
    ('I', 2, 7.5, 0.001): (3.040430023903117e-05, 0.0001693174629129439),
    ('I', 2, 7.5, 1e-06): (1.9687890928221527e-08, 0.00026616692256925897),
    ('I', 2, 7.5, 1e-09): (1.844047823475353e-11, 0.0002843444918062975),
    ('I', 2, 7.5, 1e-12): (1.8251658541721587e-14, 0.00028730069587144726),
    ('I', 2, 7.5, 'box'): (0.3663341111566629, 5.449341049301004e-06),
    ('I', 2, 64.0, 0.001): (2.10622406535263e-06, 0.00017785547710655124),
    ('I', 2, 64.0, 1e-06): (2.5746320822240383e-11, 0.0022148654744474972),
    ('I', 2, 64.0, 1e-09): (1.0617008565877689e-15, 0.010106627836447555),
    ('I', 2, 64.0, 1e-12): (9.974183935419277e-20, 0.026696324177692597),
    ('I', 2, 64.0, 'box'): (0.38714722921736383, 2.490589871239913e-06),
    ('I', 12, 1.0, 0.001): (5.9460494856894406e-08, 4.8125764921797185e-05),
    ('I', 12, 1.0, 1e-06): (5.946030388847368e-11, 4.812602621044178e-05),
    ('I', 12, 1.0, 1e-09): (5.946030388829263e-14, 4.8126026210708984e-05),
    ('I', 12, 1.0, 1e-12): (5.946030388829264e-17, 4.812602621071619e-05),
    ('I', 12, 1.0, 'box'): (0.019592401036766294, 0.00013582115975141002),
    ('I', 12, 3.0, 0.001): (1.4655579077108414e-09, 0.005730146883322072),
    ('I', 12, 3.0, 1e-06): (1.4187532392858854e-12, 0.005906550022824356),
    ('I', 12, 3.0, 1e-09): (1.4182968859081477e-15, 0.0059083224893254115),
    ('I', 12, 3.0, 1e-12): (1.418292323520706e-18, 0.0059083402148508695),
    ('I', 12, 3.0, 'box'): (0.010531259269513007, 0.00024287662747633884),
    ('I', 12, 7.5, 0.001): (1.8153541483860104e-12, 0.16988202167912717),
    ('I', 12, 7.5, 1e-06): (7.176923643985743e-16, 0.23545214148075594),
    ('I', 12, 7.5, 1e-09): (6.264084071738378e-19, 0.24539848073365703),
    ('I', 12, 7.5, 1e-12): (6.13192169354434e-22, 0.24695947351152894),
    ('I', 12, 7.5, 'box'): (0.006678102425065907, 0.00018283341196178535),
    ('I', 12, 64.0, 0.001): (6.774208792496779e-25, 0.7700385315115422),
    ('I', 12, 64.0, 1e-06): (4.5152416788957086e-39, 0.9740721508558755),
    ('I', 12, 64.0, 1e-09): (7.182346450965485e-51, 0.9945857042071419),
    ('I', 12, 64.0, 1e-12): (6.475824904954989e-61, 0.9984612985246855),
    ('I', 12, 64.0, 'box'): (0.003936563445324077, 4.189836076415604e-05),
    ('equi', 2, 3.0, 0.001): (0.00031608127170509957, 9.178845047058546e-06),
    ('equi', 2, 3.0, 1e-06): (3.1253348872635527e-07, 9.356264293828035e-06),
    ('equi', 2, 3.0, 1e-09): (3.124982684001029e-10, 9.358037911015145e-06),
    ('equi', 2, 3.0, 1e-12): (3.1249791622293015e-13, 9.358055645677555e-06),
    ('equi', 3, 3.0, 0.001): (0.00016289915432222556, 4.7305712427602496e-05),
    ('equi', 3, 3.0, 1e-06): (1.6040900786554426e-07, 3.305282952083516e-05),
    ('equi', 3, 3.0, 1e-09): (1.6038443900255514e-10, 3.305946338295902e-05),
    ('equi', 3, 3.0, 1e-12): (1.603841933404784e-13, 3.3059529718287406e-05),
}
