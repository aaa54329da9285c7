"""Single-precision FHT sum-product decoding (include/nbldpc.h, nbl_create_fht32) restated in numpy -- TEST INFRASTRUCTURE ONLY.

check_node32() is the header's check-node update, step by step, in np.float32 with the floor at 2^-NBL_FHT32_FLOOR_LOG2; it reuses
fht_ref.wht.  Fht32Check wraps it the way fht_ref.FhtCheck wraps the FP64 one, with dtype = np.float32, so that fht_ref.decode_flooding
and fht_ref.decode_layered run the whole schedule in float32 unchanged: L_ch rounded to float32 once, every sum, difference and product
of the variable side a float32 operation.

via64: the second evaluation of the parity statement.  exp and log are the only operations two implementations of the definition may
round differently (any evaluation within 2 ulp is allowed); via64=True takes them in float64 and rounds once to float32 -- a correctly
rounded float32 exp / log for all but a 2^-29 fraction of arguments -- where via64=False takes numpy's float32 functions.

D32: per (case, schedule) of tests/test_gpu_fht32.py the largest |w(x_a) - w(x_b)| over post, c2v and v2c of every frame between the two
evaluations, recorded from tests/test_fht32.py::test_conditions_on_every_gpu_case (which recomputes and compares it).  The GPU tolerance
is 16 x this figure: 4 x for a 2-ulp device function against a correctly rounded one, 4 x for sample-to-sample spread."""
import numpy as np

import fht_ref as fr

FLOOR_LOG2 = 16  # NBL_FHT32_FLOOR_LOG2
F32 = np.float32

# (case, schedule) -> D32; "gf16-fixed" = gf16 with fixed_iters = 1
D32 = {
    ("gf16", "flooding"): 5.721e-06,
    ("gf16", "greedy"): 2.937e-06,
    ("ring256", "flooding"): 7.794e-06,
    ("ring256", "greedy"): 6.590e-06,
    ("ring256", "serial"): 5.217e-06,
    ("ring256", "other"): 7.794e-06,
    ("ring64", "flooding"): 1.338e-06,
    ("ring64", "greedy"): 3.311e-05,
    ("ring64", "serial"): 3.311e-05,
    ("ring64", "other"): 2.134e-06,
    ("all-4", "flooding"): 1.003e-06,
    ("all-4", "greedy"): 3.664e-06,
    ("all-8", "flooding"): 1.518e-06,
    ("all-8", "greedy"): 2.145e-05,
    ("all-16", "flooding"): 4.028e-06,
    ("all-16", "greedy"): 4.703e-05,
    ("dv48-32", "flooding"): 3.940e-06,
    ("dv48-32", "greedy"): 2.270e-05,
    ("rand128", "flooding"): 8.502e-06,
    ("rand128", "greedy"): 5.080e-06,
    ("gf16-fixed", "flooding"): 5.721e-06,
    ("gf16-fixed", "greedy"): 3.832e-06,
}


def _exp(x, via64):
    return np.exp(x.astype(np.float64)).astype(F32) if via64 else np.exp(x)


def _log(x, via64):
    return np.log(x.astype(np.float64)).astype(F32) if via64 else np.log(x)


def transform_outputs(vin, h, gf_mul, dtype=F32, via64=False):
    """steps 1-5 in `dtype`: v [dc][q] before the floor, in the check domain (np.longdouble: what the float32 noise is measured against)"""
    dc, q = len(h), gf_mul.shape[0]
    perm = np.asarray(gf_mul)[np.asarray(h, dtype=np.int64)].astype(np.int64)
    p = np.zeros((dc, q), dtype=dtype)
    for d in range(dc):
        p[d, perm[d, 1:]] = np.asarray(vin[d], dtype=dtype)                   # 1.
    x = p - p.max(axis=1, keepdims=True)
    u = _exp(x, via64) if dtype is F32 else np.exp(x)                         # 2.
    U = fr.wht(u)                                                             # 3.
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
    return v, perm


def check_node32(vin, h, gf_mul, via64=False):
    """vin [dc][q-1] incoming LLR vectors (slot 0 implicit; rounded to float32 if they are not), h [dc] edge coefficients, gf_mul [q][q].
    Returns c2v [dc][q-1] in np.float32."""
    v, perm = transform_outputs(vin, h, gf_mul, F32, via64)
    t = v.max(axis=1, keepdims=True)                                          # 6.
    assert np.all(t > 0)
    v = np.maximum(v, t * F32(2.0 ** -FLOOR_LOG2))
    lv = _log(v, via64)
    c = lv - lv[:, :1]                                                        # 7.
    assert c.dtype == F32
    return np.stack([c[d, perm[d, 1:]] for d in range(len(h))])


def noise_over_t(vin, h, gf_mul):
    """largest |v32 - v80| / t over the outputs of one check: the transform's rounding noise relative to the vector's largest entry,
    which the floor 2^-16 has to stay well above"""
    v32, _ = transform_outputs(vin, h, gf_mul, F32)
    v80, _ = transform_outputs(np.asarray(vin, dtype=F32), h, gf_mul, np.longdouble)
    t = v80.max(axis=1, keepdims=True)
    return float(np.max(np.abs(v32.astype(np.longdouble) - v80) / t))


class Fht32Check(fr.FhtCheck):
    """fht_ref.FhtCheck with dtype = np.float32 and the float32 check node: fht_ref.decode_flooding / decode_layered on it run the whole
    schedule in float32.  via64 selects the second evaluation of exp / log."""

    def __init__(self, ocode, gf_mul, via64=False):
        super().__init__(ocode, gf_mul, F32)
        self.via64 = via64

    def check(self, m, vin):
        g = self.g
        assert np.asarray(vin).dtype == F32
        return check_node32(vin, g.c_h[g.coff[m]:g.coff[m + 1]], self.mul, self.via64)
