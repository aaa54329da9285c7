"""Single-precision FHT sum-product decoding for checks above degree 8 (include/nbldpc.h, nbl_create_fht32_wide) restated in numpy --
TEST INFRASTRUCTURE ONLY.

check_node32_scaled() is fht32_ref.check_node32 with the header's step 3a: every transformed input U_d is multiplied by the float32
power of two 2^-e_d, where 2^e_d <= U_d[0] < 2^(e_d+1) (np.frexp on slot 0).  Steps 4-7 run on the scaled vectors unchanged.
Fht32WideCheck wraps it the way fht32_ref.Fht32Check wraps the unscaled update, so that fht_ref.decode_flooding / decode_layered run the
whole schedule in float32; via64 keeps the meaning it has in fht32_ref (exp / log taken in float64 and rounded once to float32).

D32W: per (case, schedule) of tests/fht32_wide_cases.py the largest |w(x_a) - w(x_b)| over post, c2v and v2c of every frame between the
two evaluations, recorded from tests/test_fht32_wide.py::test_conditions_on_every_case (which recomputes and compares it).  The GPU
tolerance is 16 x this figure (tests/fht32_ref.py says why 16).  Keys "<case>-fixed" are fixed_iters = 1; keys "sw3:<case>" are the
cases of tests/test_fht32.py (check degrees up to 8) under the scaled update, which nbl_debug_force_generic(dec, 3) selects."""
import numpy as np

import fht_ref as fr
import fht32_ref as f32

F32 = f32.F32
FLOOR_LOG2 = f32.FLOOR_LOG2

# (case, schedule) -> D32W
D32W = {
    ("wide-256", "flooding"): 1.859e-06,
    ("wide-256", "greedy"): 2.036e-06,
    ("wide-64", "flooding"): 1.211e-06,
    ("wide-64", "greedy"): 1.372e-06,
    ("wide-128", "flooding"): 1.122e-06,
    ("wide-128", "greedy"): 1.367e-06,
    ("wide-16", "flooding"): 9.198e-07,
    ("wide-16", "greedy"): 9.498e-07,
    ("wide-4", "flooding"): 7.952e-07,
    ("wide-4", "greedy"): 1.590e-06,
    ("mix-256", "flooding"): 7.011e-07,
    ("mix-256", "greedy"): 4.684e-07,
    ("mix-16", "flooding"): 2.602e-06,
    ("mix-16", "greedy"): 5.141e-06,
    ("ring16-dc16", "flooding"): 4.360e-06,
    ("ring16-dc16-fixed", "flooding"): 4.360e-06,
    ("ring16-dc16", "greedy"): 2.936e-06,
    ("ring16-dc16-fixed", "greedy"): 3.874e-06,
    ("flat-256", "flooding"): 8.882e-07,
    ("flat-256", "greedy"): 8.882e-07,
    ("sw3:gf16", "flooding"): 3.171e-06,
    ("sw3:gf16", "greedy"): 3.277e-06,
    ("sw3:ring256", "flooding"): 4.581e-06,
    ("sw3:ring256", "greedy"): 2.689e-06,
    ("sw3:ring64", "flooding"): 1.451e-06,
    ("sw3:ring64", "greedy"): 1.187e-05,
    ("sw3:all-16", "flooding"): 1.162e-06,
    ("sw3:all-16", "greedy"): 6.838e-06,
    ("sw3:rand128", "flooding"): 3.088e-06,
    ("sw3:rand128", "greedy"): 6.030e-06,
}


def scale_of(U):
    """2^-e_d per row of U [dc][q], as float32 [dc][1]: 2^e_d <= U_d[0] < 2^(e_d+1)"""
    s0 = U[:, 0]
    assert np.all(s0 >= 1) and np.all(np.isfinite(s0.astype(np.float64)))
    _, e = np.frexp(s0.astype(np.float64))               # s0 = m 2^e, 0.5 <= m < 1: e_d = e - 1
    return np.ldexp(1.0, -(e - 1)).astype(U.dtype)[:, None]


def transform_outputs_scaled(vin, h, gf_mul, dtype=F32, via64=False, scale=None):
    """steps 1-5 with step 3a in `dtype`: v [dc][q] before the floor, in the check domain, perm, and the scales 2^-e_d used.  scale: take
    these instead of step 3a's own (np.longdouble with the float32 evaluation's scales is what the float32 noise is measured against: a
    slot 0 that lies within a rounding of a power of two may fall on either side of it in the two arithmetics)"""
    dc, q = len(h), gf_mul.shape[0]
    perm = np.asarray(gf_mul)[np.asarray(h, dtype=np.int64)].astype(np.int64)
    p = np.zeros((dc, q), dtype=dtype)
    for d in range(dc):
        p[d, perm[d, 1:]] = np.asarray(vin[d], dtype=dtype)                   # 1.
    x = p - p.max(axis=1, keepdims=True)
    u = f32._exp(x, via64) if dtype is F32 else np.exp(x)                     # 2.
    U = fr.wht(u)                                                             # 3.
    sc = scale_of(U) if scale is None else np.asarray(scale, dtype=dtype)
    U = U * sc                                                                # 3a.
    assert U.dtype == dtype
    fwd, bwd = [None] * dc, [None] * dc                                       # 4.
    fwd[1] = U[0]
    for k in range(1, dc - 1):
        fwd[k + 1] = fwd[k] * U[k]
    bwd[dc - 2] = U[dc - 1]
    for k in range(dc - 2, 0, -1):
        bwd[k - 1] = bwd[k] * U[k]
    V = np.stack([bwd[0] if d == 0 else fwd[d] if d == dc - 1 else fwd[d] * bwd[d] for d in range(dc)])
    v = fr.wht(V)                                                             # 5.
    assert v.dtype == dtype
    return v, perm, sc


def check_node32_scaled(vin, h, gf_mul, via64=False):
    """vin [dc][q-1] incoming LLR vectors (slot 0 implicit; rounded to float32 if they are not), h [dc] edge coefficients, gf_mul [q][q].
    Returns c2v [dc][q-1] in np.float32."""
    v, perm, _ = transform_outputs_scaled(vin, h, gf_mul, F32, via64)
    t = v.max(axis=1, keepdims=True)                                          # 6.
    assert np.all(t > 0)
    v = np.maximum(v, t * F32(2.0 ** -FLOOR_LOG2))
    lv = f32._log(v, via64)
    c = lv - lv[:, :1]                                                        # 7.
    assert c.dtype == F32
    return np.stack([c[d, perm[d, 1:]] for d in range(len(h))])


def noise_over_t(vin, h, gf_mul):
    """largest |v32 - v80| / t over the outputs of one check under the scaled update (fht32_ref.noise_over_t with step 3a)"""
    v32, _, sc = transform_outputs_scaled(vin, h, gf_mul, F32)
    v80, _, _ = transform_outputs_scaled(np.asarray(vin, dtype=F32), h, gf_mul, np.longdouble, scale=sc)
    t = v80.max(axis=1, keepdims=True)
    return float(np.max(np.abs(v32.astype(np.longdouble) - v80) / t))


class Fht32WideCheck(f32.Fht32Check):
    """fht32_ref.Fht32Check with the scaled check node"""

    def check(self, m, vin):
        g = self.g
        assert np.asarray(vin).dtype == F32
        return check_node32_scaled(vin, g.c_h[g.coff[m]:g.coff[m + 1]], self.mul, self.via64)
