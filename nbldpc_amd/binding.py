"""ctypes binding of the product library nbldpc_amd/csrc/libnbldpc_hip.so (C ABI: include/nbldpc.h).

This is plumbing for tests/ and bench.py.  There is no Python or CPU fallback: if the HIP library is
missing, or no GPU is present, the calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import datafiles

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NBL_HIP_LIB") or os.path.join(_HERE, "csrc", "libnbldpc_hip.so")  # NBL_HIP_LIB: A/B builds

METHOD_BP, METHOD_EMS, METHOD_TEMS, METHOD_OSD, METHOD_BS_TEMS = 1, 2, 4, 6, 7
METHOD_MINMAX = 3        # NBL_METHOD_MINMAX: through nbl_create_minmax alone (Decoder(..., minmax=True))
DEMOD_LOGSUM, DEMOD_MAXLOG = 0, 1
SOFT_LOGSUM, SOFT_MAXLOG = 0, 1
SOFT_EXTRINSIC = 1
FHT_LAYERED = 1          # NBL_FHT_LAYERED
FHT32_LAYERED = 1        # NBL_FHT32_LAYERED
FHT32_WIDE_LAYERED = 1   # NBL_FHT32_WIDE_LAYERED
EMS_WIDE_LAYERED = 1     # NBL_EMS_WIDE_LAYERED
TEMS_WIDE_LAYERED = 1    # NBL_TEMS_WIDE_LAYERED
BP_WIDE_LAYERED = 1      # NBL_BP_WIDE_LAYERED
MINMAX_LAYERED = 1       # NBL_MINMAX_LAYERED
# the entry points that name a decoder kind: the library's name of the kind -> (creation function, its layered flag)
KIND_ENTRY = {"fht": ("nbl_create_fht", FHT_LAYERED), "fht32": ("nbl_create_fht32", FHT32_LAYERED), "fht32_wide": ("nbl_create_fht32_wide", FHT32_WIDE_LAYERED),
              "ems_wide": ("nbl_create_ems_wide", EMS_WIDE_LAYERED),
              "tems_wide": ("nbl_create_tems_wide", TEMS_WIDE_LAYERED), "bp_wide": ("nbl_create_bp_wide", BP_WIDE_LAYERED),
              "minmax": ("nbl_create_minmax", MINMAX_LAYERED)}
FADING_NONE, FADING_RAYLEIGH = 0, 1

# every symbol include/nbldpc.h declares
EXPORTS = ("nbl_abi_version", "nbl_create", "nbl_create_ex", "nbl_create_osd", "nbl_layer_greedy", "nbl_create_layered", "nbl_create_layered_ex", "nbl_create_layered_bp", "nbl_create_fht", "nbl_create_ems_wide", "nbl_create_tems_wide", "nbl_create_bp_wide", "nbl_create_minmax", "nbl_get_layers", "nbl_destroy", "nbl_decode_batch", "nbl_decode_batch_device",
           "nbl_set_demodulator", "nbl_set_demodulator_ex", "nbl_decode_batch_samples", "nbl_decode_batch_noise", "nbl_rand_advance", "nbl_channel_batch", "nbl_decode_batch_resident",
           "nbl_set_transmitter", "nbl_transmit_batch", "nbl_pn_advance", "nbl_count_errors", "nbl_encode_batch", "nbl_read_transmitted",
           "nbl_read_state", "nbl_set_record_state", "nbl_set_profiling", "nbl_last_timing", "nbl_last_error",
           "nbl_workspace_bytes", "nbl_decode_batch_bits", "nbl_decode_batch_bits_device", "nbl_soft_output", "nbl_soft_output_device",
           "nbl_decode_batch_samples_prior", "nbl_soft_output_ex", "nbl_soft_output_device_ex", "nbl_decode_batch_samples_idd", "nbl_decode_batch_resident_idd",
           "nbl_decode_batch_samples_csi", "nbl_decode_batch_samples_idd_csi", "nbl_set_fading", "nbl_channel_draws", "nbl_read_gains")


class NblError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"nbldpc status {status}: {msg}")
        self.status = status


class CodeDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("M", C.c_int32), ("q", C.c_int32),
                ("var_deg", C.c_void_p), ("chk_deg", C.c_void_p), ("var_chk", C.c_void_p), ("var_h", C.c_void_p),
                ("chk_var", C.c_void_p), ("chk_h", C.c_void_p)]


class Params(C.Structure):
    _fields_ = [("method", C.c_int32), ("max_iter", C.c_int32), ("ems_nm", C.c_int32), ("ems_nc", C.c_int32),
                ("ems_factor", C.c_double), ("ems_offset", C.c_double), ("tems_nr", C.c_int32), ("tems_nc", C.c_int32),
                ("tems_factor", C.c_double), ("tems_offset", C.c_double), ("fixed_iters", C.c_int32),
                ("poll_every", C.c_int32), ("max_batch", C.c_int32)]


class ParamsExt(C.Structure):
    _fields_ = [("bs_nm", C.c_int32), ("bs_nc", C.c_int32), ("bs_factor", C.c_double), ("bs_offset", C.c_double)]


class IddParams(C.Structure):
    _fields_ = [("passes", C.c_int32), ("soft_metric", C.c_int32)]


class FadingDesc(C.Structure):
    _fields_ = [("model", C.c_int32), ("coherence", C.c_int32)]


class OsdParams(C.Structure):
    _fields_ = [("order", C.c_int32), ("flag", C.c_int32), ("factor", C.c_double), ("crc_len", C.c_int32), ("crc_rows", C.c_int32),
                ("gf_mat", C.c_void_p)]


_lib = None


def load_library():
    """Load libnbldpc_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: build it with `make -C nbldpc_amd/csrc` "
                                    "(or python -c 'import __graft_entry__ as g; g.build()')")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.  If torch is going to be used in this process
        # (bench.py, tests) it must be loaded BEFORE our library so that both resolve to the same runtime instance; loading
        # ours first makes a later torch.cuda initialisation fail with "No HIP GPUs are available".
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        L.nbl_abi_version.restype = C.c_int32
        L.nbl_create.restype = C.c_int
        L.nbl_create.argtypes = [C.POINTER(CodeDesc), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]
        L.nbl_create_ex.restype = C.c_int
        L.nbl_create_ex.argtypes = [C.POINTER(CodeDesc), C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(ParamsExt), C.c_int,
                                    C.POINTER(C.c_void_p)]
        L.nbl_create_osd.restype = C.c_int
        L.nbl_create_osd.argtypes = [C.POINTER(CodeDesc), C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(ParamsExt),
                                     C.POINTER(OsdParams), C.c_int, C.POINTER(C.c_void_p)]
        L.nbl_layer_greedy.restype = C.c_int32
        L.nbl_layer_greedy.argtypes = [C.POINTER(CodeDesc), C.c_void_p]
        L.nbl_create_layered.restype = C.c_int
        L.nbl_create_layered.argtypes = [C.POINTER(CodeDesc), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.nbl_create_layered_ex.restype = C.c_int
        L.nbl_create_layered_ex.argtypes = [C.POINTER(CodeDesc), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.nbl_create_layered_bp.restype = C.c_int
        L.nbl_create_layered_bp.argtypes = [C.POINTER(CodeDesc), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        for fn, _ in KIND_ENTRY.values():   # one signature: (code, gf_mul, gf_inv, params, layer_of, flags, device, out)
            if not hasattr(L, fn):          # (an NBL_HIP_LIB built from an older commit: the kind is an AttributeError where it is asked for)
                continue
            getattr(L, fn).restype = C.c_int
            getattr(L, fn).argtypes = [C.POINTER(CodeDesc), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.nbl_get_layers.restype = C.c_int
        L.nbl_get_layers.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        L.nbl_destroy.argtypes = [C.c_void_p]
        L.nbl_destroy.restype = None
        L.nbl_decode_batch.restype = C.c_int
        L.nbl_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_decode_batch_device.restype = C.c_int
        L.nbl_decode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_decode_batch_bits.restype = C.c_int
        L.nbl_decode_batch_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_decode_batch_bits_device.restype = C.c_int
        L.nbl_decode_batch_bits_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_soft_output.restype = C.c_int
        L.nbl_soft_output.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.nbl_soft_output_device.restype = C.c_int
        L.nbl_soft_output_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_soft_output_ex.restype = C.c_int
        L.nbl_soft_output_ex.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.nbl_soft_output_device_ex.restype = C.c_int
        L.nbl_soft_output_device_ex.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_decode_batch_samples_prior.restype = C.c_int
        L.nbl_decode_batch_samples_prior.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_decode_batch_samples_idd.restype = C.c_int
        L.nbl_decode_batch_samples_idd.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.POINTER(IddParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_decode_batch_resident_idd.restype = C.c_int
        L.nbl_decode_batch_resident_idd.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.POINTER(IddParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_decode_batch_samples_csi.restype = C.c_int
        L.nbl_decode_batch_samples_csi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_decode_batch_samples_idd_csi.restype = C.c_int
        L.nbl_decode_batch_samples_idd_csi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.POINTER(IddParams), C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]
        L.nbl_set_fading.restype = C.c_int
        L.nbl_set_fading.argtypes = [C.c_void_p, C.POINTER(FadingDesc)]
        L.nbl_channel_draws.restype = C.c_uint64
        L.nbl_channel_draws.argtypes = [C.c_void_p]
        L.nbl_read_gains.restype = C.c_int
        L.nbl_read_gains.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.nbl_read_state.restype = C.c_int
        L.nbl_read_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_set_record_state.argtypes = [C.c_void_p, C.c_int32]
        L.nbl_set_profiling.argtypes = [C.c_void_p, C.c_int32]
        L.nbl_last_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.nbl_last_error.restype = C.c_char_p
        L.nbl_last_error.argtypes = [C.c_void_p]
        L.nbl_workspace_bytes.restype = C.c_size_t
        L.nbl_workspace_bytes.argtypes = [C.c_void_p]
        _lib = L
    return _lib


class Code:
    """Tanner graph in the reference's file order (both directions), 0-based."""

    def __init__(self, name=None, spec=None):
        c = spec if spec is not None else datafiles.codes()[name]
        self.name = name
        self.N, self.M, self.q = c["N"], c["M"], c["q"]
        self.var_deg = np.array([len(r) for r in c["var_rows"]], dtype=np.int32)
        self.chk_deg = np.array([len(r) for r in c["chk_rows"]], dtype=np.int32)
        self.var_chk = np.array([x[0] - 1 for r in c["var_rows"] for x in r], dtype=np.int32)
        self.var_h = np.array([x[1] for r in c["var_rows"] for x in r], dtype=np.int32)
        self.chk_var = np.array([x[0] - 1 for r in c["chk_rows"] for x in r], dtype=np.int32)
        self.chk_h = np.array([x[1] for r in c["chk_rows"] for x in r], dtype=np.int32)
        self.E = int(self.var_deg.sum())

    def desc(self):
        return CodeDesc(self.N, self.M, self.q, self.var_deg.ctypes.data, self.chk_deg.ctypes.data,
                        self.var_chk.ctypes.data, self.var_h.ctypes.data, self.chk_var.ctypes.data, self.chk_h.ctypes.data)


def layer_greedy(code):
    """The library's default layer assignment of the layered schedule (nbl_layer_greedy; host arithmetic, no device):
    layer_of [M] int32.  Checks in ascending index, each in the smallest layer that holds no check sharing a variable with it."""
    lib = load_library()
    layer_of = np.zeros(code.M, dtype=np.int32)
    desc = code.desc()
    rc = lib.nbl_layer_greedy(C.byref(desc), layer_of.ctypes.data)
    if rc < 0:
        raise NblError(rc, lib.nbl_last_error(None).decode())
    assert rc == int(layer_of.max()) + 1
    return layer_of


class PlanInfo(C.Structure):
    _fields_ = [("cn", C.c_char_p), ("fusable", C.c_int32), ("fused", C.c_int32), ("want_v2c", C.c_int32)]


def debug_plan(code, method, ems_nm=32, ems_nc=3, tems_nr=2, tems_nc=3, bs_nm=None, bs_nc=2, layers=None, damped=None,
               force_generic=0, record_state=False, fht=False, wide=False, tems_wide=False, bp_wide=False, fht32=False, fht32_wide=False, minmax=False):
    """The check-node kernel a decoder of this description would run (nbl_debug_plan; host arithmetic, no device, no decoder):
    (kernel name, fusable, fused, want_v2c).  The description is built the way Decoder builds it; layers / damped / fht as there
    (None = flooding), force_generic as nbl_debug_force_generic takes it (with fht, 3 names the wide programme, fht_wide /
    fht_wide_layered, at any check degree; with wide, the decoder nbl_create_ems_wide would make: 3 names ems_wide / ems_wide_layered at
    any check degree; with tems_wide, the decoder nbl_create_tems_wide would make: 3 names tems_wide / tems_wide_layered at any check
    degree where tems_nc <= 4; with bp_wide, the decoder nbl_create_bp_wide would make: 3 names bp_wide / bp_wide_layered at any check
    degree; with fht32, the decoder nbl_create_fht32 would make: fht32 / fht32_layered under every switch; with fht32_wide, the decoder
    nbl_create_fht32_wide would make: 3 names fht32_wide / fht32_wide_layered at any check degree), record_state as
    nbl_set_record_state; with minmax (method 3), the decoder nbl_create_minmax would make: minmax / minmax_layered under every switch.
    fht, wide, tems_wide, bp_wide, fht32, fht32_wide and minmax exclude one another."""
    kinds = [k for k, on in dict(fht=fht, ems_wide=wide, tems_wide=tems_wide, bp_wide=bp_wide, fht32=fht32, fht32_wide=fht32_wide, minmax=minmax).items() if on]
    if len(kinds) > 1:
        raise ValueError("fht, wide, tems_wide, bp_wide, fht32, fht32_wide and minmax name seven different entry points: give one of them")
    lib = load_library()
    params = Params(method, 0, ems_nm, ems_nc, 1.0, 0.0, tems_nr, tems_nc, 1.0, 0.0, 0, 0, 0)
    ext = ParamsExt(bs_nm, bs_nc, 1.0, 0.0) if bs_nm is not None else None
    desc = code.desc()
    out = PlanInfo()
    if kinds:   # the library resolves the name: no enum is mirrored here
        fn = "nbl_debug_plan_kind"
        lib.nbl_debug_plan_kind.restype = C.c_int
        lib.nbl_debug_plan_kind.argtypes = [C.POINTER(CodeDesc), C.POINTER(Params), C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PlanInfo)]
        rc = lib.nbl_debug_plan_kind(C.byref(desc), C.byref(params), kinds[0].encode(), int(layers is not None), force_generic, int(record_state), C.byref(out))
    else:
        fn = "nbl_debug_plan"
        lib.nbl_debug_plan.restype = C.c_int
        lib.nbl_debug_plan.argtypes = [C.POINTER(CodeDesc), C.POINTER(Params), C.POINTER(ParamsExt), C.c_int32, C.c_int32, C.c_int32, C.POINTER(PlanInfo)]
        rc = lib.nbl_debug_plan(C.byref(desc), C.byref(params), C.byref(ext) if ext is not None else None,
                                -1 if layers is None else int(bool(damped)), force_generic, int(record_state), C.byref(out))
    if rc != 0:
        raise NblError(rc, fn)
    return out.cn.decode(), bool(out.fusable), bool(out.fused), bool(out.want_v2c)


class Decoder:
    """Batched decoder handle (nbl_create .. nbl_destroy).  Basic-set T-EMS (method 7) takes bs_nm / bs_nc / bs_factor / bs_offset
    through nbl_create_ex; without bs_nm the handle is made by nbl_create, which refuses method 7.  OSD (method 6, or post-processing
    of methods 1/2/4/7 with osd_order >= 0) takes osd_* / crc_len / crc_rows / gf_mat through nbl_create_osd; with osd_order=None the
    handle is made as before, so method 6 is refused.  gf_mat=None: the GF element matrices as the reference's loader leaves them
    (datafiles.gf_matrices(q, as_loaded=True)).  layers: None = the flooding schedule; "greedy" or an int array [M] (a layer per
    check) = the layered schedule through nbl_create_layered (EMS only; no bs_* / osd_* parameters go with it).  damped (with layers
    only): None = nbl_create_layered as before; anything else goes through nbl_create_layered_ex with flags = int(damped), so True =
    NBL_LAYERED_DAMPED: T-EMS under the layered schedule with its per-edge damping (inert for EMS), False = flags 0.  bp=True (with
    layers, without damped): nbl_create_layered_bp, log-QSPA under the layered schedule with its 0.5 / 0.5 per-edge damping.  fht=True (method 1
    only; without damped, bp, OSD or extension parameters): nbl_create_fht, the FHT sum-product check node in place of the exact one --
    flooding without layers, the layered schedule of nbl_create_layered_bp with layers="greedy" or an assignment; it takes
    checks above degree 8 (up to NBL_FHT_MAX_CHECK_DEGREE = 32: high-rate codes), with no argument of its own; so do wide=True, for EMS, and tems_wide=True, for T-EMS.  wide=True (method 2 only;
    without damped, bp, fht, OSD or extension parameters): nbl_create_ems_wide, the EMS decoder of nbl_create (without layers) or of
    nbl_create_layered (layers="greedy" or an assignment) with check degrees up to NBL_EMS_MAX_CHECK_DEGREE = 32.  tems_wide=True (method 4
    only; without wide, damped, bp, fht, OSD or extension parameters): nbl_create_tems_wide, the T-EMS decoder of nbl_create (without
    layers) or of nbl_create_layered_ex with NBL_LAYERED_DAMPED (layers="greedy" or an assignment) with check degrees up to
    NBL_TEMS_MAX_CHECK_DEGREE = 32 over any field and tems_nc up to 4 there.  bp_wide=True (method 1 only; without fht, wide, tems_wide,
    damped, bp, OSD or extension parameters): nbl_create_bp_wide, the exact log-QSPA decoder of nbl_create (without layers) or of
    nbl_create_layered_bp (layers="greedy" or an assignment) with check degrees up to NBL_BP_MAX_CHECK_DEGREE = 32.  fht32=True (method 1
    only; without fht, bp, damped, wide, tems_wide, bp_wide, OSD or extension parameters): nbl_create_fht32, the FHT decoder in single
    precision -- float messages, the floor at 2^-16, check degrees up to 8 -- flooding without layers, layered with layers="greedy" or an
    assignment; read_state and soft_output return doubles that are the exact widening of the float state.  fht32_wide=True (method 1
    only; without any of the other kind flags, bp, damped, OSD or extension parameters): nbl_create_fht32_wide, the same decoder with check
    degrees up to NBL_FHT32_MAX_CHECK_DEGREE = 32 (a code with a check above degree 8 runs the update with every transformed input scaled
    by a power of two).  minmax=True (method 3, METHOD_MINMAX, only; without any of the other kind flags, bp, damped, OSD or extension
    parameters): nbl_create_minmax, Min-Max decoding with check degrees up to NBL_MINMAX_MAX_CHECK_DEGREE = 32 -- flooding without layers,
    the layered schedule of nbl_create_layered with layers="greedy" or an assignment; ems_factor / ems_offset shape its c2v messages.
    Without the flag method 3 goes to nbl_create, which refuses it."""

    def __init__(self, code, method, max_iter, ems_nm=32, ems_nc=3, ems_factor=1.0, ems_offset=0.0, tems_nr=2, tems_nc=3,
                 tems_factor=1.0, tems_offset=0.0, fixed_iters=0, poll_every=0, max_batch=0, device=0, gf=None,
                 bs_nm=None, bs_nc=2, bs_factor=1.0, bs_offset=0.0, osd_order=None, osd_flag=0, osd_factor=0.0, crc_len=8, crc_rows=0,
                 gf_mat=None, layers=None, damped=None, bp=False, fht=False, wide=False, tems_wide=False, bp_wide=False, fht32=False, fht32_wide=False, minmax=False):
        self.lib = load_library()
        self.code = code
        mul, inv = gf if gf is not None else datafiles.gf_tables(code.q)
        self._mul = np.ascontiguousarray(np.array(mul, dtype=np.uint16))
        self._inv = np.ascontiguousarray(np.array(inv, dtype=np.uint16))
        self.params = Params(method, max_iter, ems_nm, ems_nc, ems_factor, ems_offset, tems_nr, tems_nc, tems_factor,
                             tems_offset, fixed_iters, poll_every, max_batch)
        desc = code.desc()
        h = C.c_void_p()
        if damped is not None and layers is None:
            raise ValueError("damped: the flag belongs to the layered schedule (give layers='greedy' or an assignment)")
        if bp and layers is None:
            raise ValueError("bp: nbl_create_layered_bp is a layered schedule (give layers='greedy' or an assignment)")
        if bp and damped is not None:
            raise ValueError("bp: nbl_create_layered_bp takes no flags (its damping is part of the schedule): leave damped out")
        if fht and (bp or damped is not None or osd_order is not None or bs_nm is not None):
            raise ValueError("fht: nbl_create_fht takes no damped / bp flag and neither OSD nor extension parameters (layers alone picks its schedule)")
        if wide and (fht or bp or damped is not None or osd_order is not None or bs_nm is not None):
            raise ValueError("wide: nbl_create_ems_wide takes no damped / bp / fht flag and neither OSD nor extension parameters (layers alone picks its schedule)")
        if tems_wide and (wide or fht or bp or damped is not None or osd_order is not None or bs_nm is not None):
            raise ValueError("tems_wide: nbl_create_tems_wide takes no wide / damped / bp / fht flag and neither OSD nor extension parameters (layers alone picks its "
                             "schedule; the layered one is the damped one)")
        if bp_wide and (fht or wide or tems_wide):
            raise ValueError("bp_wide: fht, wide and tems_wide name other entry points (nbl_create_fht, nbl_create_ems_wide, nbl_create_tems_wide): give one of them")
        if bp_wide and (bp or damped is not None or osd_order is not None or bs_nm is not None):
            raise ValueError("bp_wide: nbl_create_bp_wide takes no damped / bp flag and neither OSD nor extension parameters (layers alone picks its schedule; "
                             "the layered one is that of nbl_create_layered_bp)")
        if fht32 and (fht or bp or damped is not None or wide or tems_wide or bp_wide or osd_order is not None or bs_nm is not None):
            raise ValueError("fht32: nbl_create_fht32 takes no fht / bp / damped / wide / tems_wide / bp_wide flag and neither OSD nor extension parameters "
                             "(layers alone picks its schedule)")
        if fht32_wide and (fht32 or fht or bp or damped is not None or wide or tems_wide or bp_wide or osd_order is not None or bs_nm is not None):
            raise ValueError("fht32_wide: nbl_create_fht32_wide takes no fht32 / fht / bp / damped / wide / tems_wide / bp_wide flag and neither OSD nor extension "
                             "parameters (layers alone picks its schedule)")
        if minmax and (fht32_wide or fht32 or fht or bp or damped is not None or wide or tems_wide or bp_wide or osd_order is not None or bs_nm is not None):
            raise ValueError("minmax: nbl_create_minmax takes no fht32_wide / fht32 / fht / bp / damped / wide / tems_wide / bp_wide flag and neither OSD nor "
                             "extension parameters (layers alone picks its schedule)")
        lay = None
        if layers is not None:
            if osd_order is not None or bs_nm is not None:
                raise ValueError("layers: nbl_create_layered takes neither OSD nor extension parameters")
            self._layer_of = None if isinstance(layers, str) and layers == "greedy" else np.ascontiguousarray(layers, dtype=np.int32)
            if self._layer_of is not None and self._layer_of.shape != (code.M,):
                raise ValueError(f"layers must be 'greedy' or one layer per check ({code.M}), got shape {self._layer_of.shape}")
            lay = None if self._layer_of is None else self._layer_of.ctypes.data
        # (at most one of the kinds: every pair is refused above)
        kinds = [k for k, on in dict(fht=fht, ems_wide=wide, tems_wide=tems_wide, bp_wide=bp_wide, fht32=fht32, fht32_wide=fht32_wide, minmax=minmax).items() if on]
        if kinds:
            fn, layered_flag = KIND_ENTRY[kinds[0]]
            rc = getattr(self.lib, fn)(C.byref(desc), self._mul.ctypes.data, self._inv.ctypes.data, C.byref(self.params), lay,
                                       0 if layers is None else layered_flag, device, C.byref(h))
        elif layers is not None and bp:
            rc = self.lib.nbl_create_layered_bp(C.byref(desc), self._mul.ctypes.data, self._inv.ctypes.data, C.byref(self.params), lay, device, C.byref(h))
        elif layers is not None and damped is None:
            rc = self.lib.nbl_create_layered(C.byref(desc), self._mul.ctypes.data, self._inv.ctypes.data, C.byref(self.params), lay, device, C.byref(h))
        elif layers is not None:
            rc = self.lib.nbl_create_layered_ex(C.byref(desc), self._mul.ctypes.data, self._inv.ctypes.data, C.byref(self.params), lay,
                                                int(damped), device, C.byref(h))
        elif osd_order is not None:
            self._gf_mat = np.ascontiguousarray(datafiles.gf_matrices(code.q) if gf_mat is None else gf_mat, dtype=np.uint8)
            self.osd = OsdParams(osd_order, osd_flag, osd_factor, crc_len, crc_rows, self._gf_mat.ctypes.data)
            self.ext = ParamsExt(bs_nm, bs_nc, bs_factor, bs_offset) if bs_nm is not None else None
            rc = self.lib.nbl_create_osd(C.byref(desc), self._mul.ctypes.data, self._inv.ctypes.data, C.byref(self.params),
                                         C.byref(self.ext) if self.ext is not None else None, C.byref(self.osd), device, C.byref(h))
        elif bs_nm is None:
            rc = self.lib.nbl_create(C.byref(desc), self._mul.ctypes.data, self._inv.ctypes.data, C.byref(self.params), device, C.byref(h))
        else:
            self.ext = ParamsExt(bs_nm, bs_nc, bs_factor, bs_offset)
            rc = self.lib.nbl_create_ex(C.byref(desc), self._mul.ctypes.data, self._inv.ctypes.data, C.byref(self.params),
                                        C.byref(self.ext), device, C.byref(h))
        if rc != 0:
            raise NblError(rc, self.lib.nbl_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.nbl_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @property
    def layers(self):
        """The layer assignment in use, [M] int32 (nbl_get_layers); None on a flooding decoder."""
        layer_of = np.zeros(self.code.M, dtype=np.int32)
        n = C.c_int32(0)
        if self.lib.nbl_get_layers(self.h, layer_of.ctypes.data, C.byref(n)) != 0:
            return None
        assert n.value == int(layer_of.max()) + 1
        return layer_of

    def _chk(self, rc):
        if rc != 0:
            raise NblError(rc, self.lib.nbl_last_error(self.h).decode())

    def decode(self, L_ch):
        """L_ch: host array [B][N][q-1] float64 -> (out[B][N] int32, converged[B] uint8, iters[B] int32)"""
        L_ch = np.ascontiguousarray(L_ch, dtype=np.float64)
        B = L_ch.shape[0]
        assert L_ch.shape == (B, self.code.N, self.code.q - 1), L_ch.shape
        out = np.zeros((B, self.code.N), dtype=np.int32)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.zeros(B, dtype=np.int32)
        self._chk(self.lib.nbl_decode_batch(self.h, L_ch.ctypes.data, B, out.ctypes.data, conv.ctypes.data, iters.ctypes.data))
        return out, conv, iters

    def decode_device(self, d_L_ch, B, d_out, d_conv=None, d_iters=None, stream=None):
        """Raw device pointers (ints); asynchronous on `stream` (a hipStream_t as int, None = decoder stream)."""
        self._chk(self.lib.nbl_decode_batch_device(self.h, d_L_ch, B, d_out, d_conv, d_iters, stream))

    def decode_bits(self, bit_llr):
        """bit_llr: host array [B][N p] float64, ln P(bit = 1) / P(bit = 0), bit j of a symbol has value 2^j -> (out, converged, iters);
        L_ch is expanded on the device (nbl_decode_batch_bits)"""
        bit_llr = np.ascontiguousarray(bit_llr, dtype=np.float64)
        B = bit_llr.shape[0]
        assert bit_llr.shape == (B, self.code.N * (self.code.q.bit_length() - 1)), bit_llr.shape
        out = np.zeros((B, self.code.N), dtype=np.int32)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.zeros(B, dtype=np.int32)
        self._chk(self.lib.nbl_decode_batch_bits(self.h, bit_llr.ctypes.data, B, out.ctypes.data, conv.ctypes.data, iters.ctypes.data))
        return out, conv, iters

    def decode_bits_device(self, d_bit_llr, B, d_out, d_conv=None, d_iters=None, stream=None):
        """Raw device pointers (ints); asynchronous on `stream` (a hipStream_t as int, None = decoder stream)."""
        self._chk(self.lib.nbl_decode_batch_bits_device(self.h, d_bit_llr, B, d_out, d_conv, d_iters, stream))

    def soft_output(self, metric="maxlog", sym=True, bits=True, B=None, extrinsic=False):
        """A-posteriori LLRs of the last decode call (nbl_soft_output): (sym_llr [B][N][q-1] | None, bit_llr [B][N p] | None).
        metric: "maxlog" / "logsum" or SOFT_MAXLOG / SOFT_LOGSUM.  B: the batch of that call; needed only when the call did not go
        through this object's decode methods (the device forms).  extrinsic: False = nbl_soft_output; anything else goes through
        nbl_soft_output_ex with flags = int(extrinsic), so True = SOFT_EXTRINSIC: the sum of the c2v alone, without the channel term."""
        m = {"maxlog": SOFT_MAXLOG, "logsum": SOFT_LOGSUM}.get(metric, metric)
        B = max(self._last_B() if B is None else B, 1)       # (before the first decode the call is refused; the buffers only have to exist)
        S = np.zeros((B, self.code.N, self.code.q - 1)) if sym else None
        Lb = np.zeros((B, self.code.N * (self.code.q.bit_length() - 1))) if bits else None
        if extrinsic is False:
            self._chk(self.lib.nbl_soft_output(self.h, int(m), S.ctypes.data if sym else None, Lb.ctypes.data if bits else None))
        else:
            self._chk(self.lib.nbl_soft_output_ex(self.h, int(m), int(extrinsic), S.ctypes.data if sym else None, Lb.ctypes.data if bits else None))
        return S, Lb

    def soft_output_device(self, metric, d_sym_llr, d_bit_llr, stream=None, extrinsic=False):
        """Raw device pointers (ints, None = that output is not wanted); enqueued on `stream`, not synchronised.  extrinsic as in
        soft_output (nbl_soft_output_device_ex)."""
        m = {"maxlog": SOFT_MAXLOG, "logsum": SOFT_LOGSUM}.get(metric, metric)
        if extrinsic is False:
            self._chk(self.lib.nbl_soft_output_device(self.h, int(m), d_sym_llr, d_bit_llr, stream))
        else:
            self._chk(self.lib.nbl_soft_output_device_ex(self.h, int(m), int(extrinsic), d_sym_llr, d_bit_llr, stream))

    def _last_B(self):
        """batch size of the last decode call (nbl_debug_last_batch; 0 before the first)"""
        self.lib.nbl_debug_last_batch.restype = C.c_int32
        self.lib.nbl_debug_last_batch.argtypes = [C.c_void_p]
        return int(self.lib.nbl_debug_last_batch(self.h))

    def set_demodulator(self, mod_order, n_mod_sym, src, constellation=None, metric=None, force_general=False):
        """src: int32 sample index per code bit (BPSK) / per code symbol (q-ary), -1 = punctured.  Any other order (and every order
        with force_general): the general demodulator, src = label-bit index per code bit [N p], -1 = not transmitted, metric
        DEMOD_LOGSUM (also None) or DEMOD_MAXLOG.  metric=None without force_general goes through nbl_set_demodulator."""
        class Demod(C.Structure):
            _fields_ = [("mod_order", C.c_int32), ("n_mod_sym", C.c_int32), ("constellation", C.c_void_p), ("src", C.c_void_p)]

        class DemodExt(C.Structure):
            _fields_ = [("metric", C.c_int32), ("force_general", C.c_int32)]
        dm_src = np.ascontiguousarray(src, dtype=np.int32)
        dm_cons = None if constellation is None else np.ascontiguousarray(constellation, dtype=np.float64)
        d = Demod(mod_order, n_mod_sym, None if dm_cons is None else dm_cons.ctypes.data, dm_src.ctypes.data)
        if metric is None and not force_general:
            self.lib.nbl_set_demodulator.argtypes = [C.c_void_p, C.c_void_p]
            self._chk(self.lib.nbl_set_demodulator(self.h, C.byref(d)))
        else:
            ext = DemodExt(DEMOD_LOGSUM if metric is None else int(metric), int(bool(force_general)))
            self.lib.nbl_set_demodulator_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            self._chk(self.lib.nbl_set_demodulator_ex(self.h, C.byref(d), C.byref(ext)))
        self._dm_src, self._dm_cons = dm_src, dm_cons
        self._tx_L = n_mod_sym

    def decode_samples(self, rx, sigma, prior=None, gain=None):
        """rx: [B][L][2] received samples -> (out, converged, iters); L_ch is built on the device.  prior: None, or [B][N p] bit LLRs
        ln P(1) / P(0) per code bit for the general demodulator (nbl_decode_batch_samples_prior).  gain: None, or [B][L][2] complex
        channel gains, one per sample (nbl_decode_batch_samples_csi)."""
        rx = np.ascontiguousarray(rx, dtype=np.float64)
        B = rx.shape[0]
        out = np.zeros((B, self.code.N), dtype=np.int32)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.zeros(B, dtype=np.int32)
        if gain is not None:
            gain = np.ascontiguousarray(gain, dtype=np.float64)
            assert gain.shape == rx.shape and rx.ndim == 3 and rx.shape[2] == 2, (gain.shape, rx.shape)
            if prior is not None:
                prior = np.ascontiguousarray(prior, dtype=np.float64)
                assert prior.shape == (B, self.code.N * (self.code.q.bit_length() - 1)), prior.shape
            self._chk(self.lib.nbl_decode_batch_samples_csi(self.h, rx.ctypes.data, gain.ctypes.data, None if prior is None else prior.ctypes.data, sigma, B,
                                                            out.ctypes.data, conv.ctypes.data, iters.ctypes.data))
            return out, conv, iters
        if prior is not None:
            prior = np.ascontiguousarray(prior, dtype=np.float64)
            assert prior.shape == (B, self.code.N * (self.code.q.bit_length() - 1)), prior.shape
            self._chk(self.lib.nbl_decode_batch_samples_prior(self.h, rx.ctypes.data, prior.ctypes.data, sigma, B, out.ctypes.data, conv.ctypes.data,
                                                              iters.ctypes.data))
            return out, conv, iters
        self.lib.nbl_decode_batch_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.nbl_decode_batch_samples(self.h, rx.ctypes.data, sigma, B, out.ctypes.data, conv.ctypes.data, iters.ctypes.data))
        return out, conv, iters

    def decode_samples_idd(self, rx, sigma, passes, soft="maxlog", gain=None):
        """Iterative demapping (nbl_decode_batch_samples_idd): up to `passes` rounds of prior-aware demodulator + decode per codeword,
        the prior of a round being the extrinsic bit LLRs (metric `soft`) of the round before -> (out, converged, iters, passes_used).
        gain: None, or [B][L][2] channel gains for the demodulator of every pass (nbl_decode_batch_samples_idd_csi)."""
        rx = np.ascontiguousarray(rx, dtype=np.float64)
        B = rx.shape[0]
        out = np.zeros((B, self.code.N), dtype=np.int32)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.zeros(B, dtype=np.int32)
        used = np.zeros(B, dtype=np.int32)
        idd = IddParams(int(passes), int({"maxlog": SOFT_MAXLOG, "logsum": SOFT_LOGSUM}.get(soft, soft)))
        if gain is not None:
            gain = np.ascontiguousarray(gain, dtype=np.float64)
            assert gain.shape == rx.shape and rx.ndim == 3 and rx.shape[2] == 2, (gain.shape, rx.shape)
            self._chk(self.lib.nbl_decode_batch_samples_idd_csi(self.h, rx.ctypes.data, gain.ctypes.data, sigma, B, C.byref(idd), out.ctypes.data,
                                                                conv.ctypes.data, iters.ctypes.data, used.ctypes.data))
            return out, conv, iters, used
        self._chk(self.lib.nbl_decode_batch_samples_idd(self.h, rx.ctypes.data, sigma, B, C.byref(idd), out.ctypes.data, conv.ctypes.data,
                                                        iters.ctypes.data, used.ctypes.data))
        return out, conv, iters, used

    def set_fading(self, model=None, coherence=1):
        """The device-side channel's fading (nbl_set_fading): model None / "awgn" / FADING_NONE = AWGN, "rayleigh" / FADING_RAYLEIGH =
        Rayleigh block fading with `coherence` consecutive samples per gain"""
        m = {None: FADING_NONE, "awgn": FADING_NONE, "none": FADING_NONE, "rayleigh": FADING_RAYLEIGH}.get(model, model)
        if m == FADING_NONE:
            self._chk(self.lib.nbl_set_fading(self.h, None))
        else:
            f = FadingDesc(int(m), int(coherence))
            self._chk(self.lib.nbl_set_fading(self.h, C.byref(f)))

    def channel_draws(self):
        """uniform draws one frame of the device-side channel moves a lane's generator (nbl_channel_draws)"""
        return int(self.lib.nbl_channel_draws(self.h))

    def read_gains(self, slot, b0, n):
        """the channel gains [n][L][2] a slot holds beside its samples (nbl_read_gains); refused on a slot without gains"""
        gain = np.zeros((n, self._tx_L, 2))
        self._chk(self.lib.nbl_read_gains(self.h, slot, b0, n, gain.ctypes.data))
        return gain

    def time_demod(self, slot, sigma, B, with_prior=False, with_gain=False):
        """diagnostic: device milliseconds of one demodulator launch on the samples a slot holds (nbl_debug_time_demod_csi)"""
        ms = C.c_double(0)
        self.lib.nbl_debug_time_demod_csi.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        self._chk(self.lib.nbl_debug_time_demod_csi(self.h, slot, sigma, B, int(with_prior), int(with_gain), C.byref(ms)))
        return ms.value

    def decode_noise(self, tx_index, lane_state, sigma):
        """tx_index [B][L] uint8, lane_state [B][3] uint32 (CRand state before the frame): channel + demodulator + decode on the device"""
        tx_index = np.ascontiguousarray(tx_index, dtype=np.uint8)
        lane_state = np.ascontiguousarray(lane_state, dtype=np.uint32)
        B = tx_index.shape[0]
        out = np.zeros((B, self.code.N), dtype=np.int32)
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.zeros(B, dtype=np.int32)
        self.lib.nbl_decode_batch_noise.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.nbl_decode_batch_noise(self.h, tx_index.ctypes.data, lane_state.ctypes.data, sigma, B, out.ctypes.data, conv.ctypes.data, iters.ctypes.data))
        return out, conv, iters

    def channel_batch(self, slot, tx_index, lane_state, sigma):
        tx_index = np.ascontiguousarray(tx_index, dtype=np.uint8)
        lane_state = np.ascontiguousarray(lane_state, dtype=np.uint32)
        self.lib.nbl_channel_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int32]
        self._chk(self.lib.nbl_channel_batch(self.h, slot, tx_index.ctypes.data, lane_state.ctypes.data, sigma, tx_index.shape[0]))

    def decode_resident(self, slot, sigma, B, want_out=True, passes=1, soft="maxlog"):
        """want_out=False: out_sym = NULL (legal once a transmitter is set), the first element returned is None.  passes=1 (an int):
        nbl_decode_batch_resident, three values; anything else goes through nbl_decode_batch_resident_idd and a fourth value,
        passes_used, is returned"""
        out = np.zeros((B, self.code.N), dtype=np.int32) if want_out else None
        conv = np.zeros(B, dtype=np.uint8)
        iters = np.zeros(B, dtype=np.int32)
        if passes != 1:
            used = np.zeros(B, dtype=np.int32)
            idd = IddParams(int(passes), int({"maxlog": SOFT_MAXLOG, "logsum": SOFT_LOGSUM}.get(soft, soft)))
            self._chk(self.lib.nbl_decode_batch_resident_idd(self.h, slot, sigma, B, C.byref(idd), out.ctypes.data if want_out else None,
                                                             conv.ctypes.data, iters.ctypes.data, used.ctypes.data))
            return out, conv, iters, used
        self.lib.nbl_decode_batch_resident.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.nbl_decode_batch_resident(self.h, slot, sigma, B, out.ctypes.data if want_out else None, conv.ctypes.data, iters.ctypes.data))
        return out, conv, iters

    def set_transmitter(self, gen, crc_len, random_msg, parallel, punct, mod_order, n_mod_sym):
        """gen [N][K] uint16 (None with random_msg = 0); punct: punctured symbol positions, ascending"""
        class TxDesc(C.Structure):
            _fields_ = [("gen", C.c_void_p), ("crc_len", C.c_int32), ("random_msg", C.c_int32), ("parallel", C.c_int32), ("punct", C.c_void_p),
                        ("n_punct", C.c_int32), ("mod_order", C.c_int32), ("n_mod_sym", C.c_int32)]
        self._tx_gen = None if gen is None else np.ascontiguousarray(gen, dtype=np.uint16)
        self._tx_punct = np.ascontiguousarray(punct, dtype=np.int32)
        t = TxDesc(None if self._tx_gen is None else self._tx_gen.ctypes.data, crc_len, random_msg, parallel,
                   self._tx_punct.ctypes.data if self._tx_punct.size else None, self._tx_punct.size, mod_order, n_mod_sym)
        self._tx_L = n_mod_sym
        self.lib.nbl_set_transmitter.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(self.lib.nbl_set_transmitter(self.h, C.byref(t)))

    def transmit_batch(self, slot, pn_state, lane_state, sigma):
        pn_state = np.ascontiguousarray(pn_state, dtype=np.uint16)
        lane_state = np.ascontiguousarray(lane_state, dtype=np.uint32)
        self.lib.nbl_transmit_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int32]
        rc = self.lib.nbl_transmit_batch(self.h, slot, pn_state.ctypes.data, lane_state.ctypes.data, sigma, pn_state.shape[0])
        self._chk(rc)

    def read_transmitted(self, slot, b0, n):
        """(tx_msg [n][K], tx_code [n][N], tx_index [n][L]) of lanes b0 .. b0 + n - 1 of a slot"""
        N, K = self.code.N, self.code.N - self.code.M
        msg = np.zeros((n, K), dtype=np.int32)
        cw = np.zeros((n, N), dtype=np.int32)
        txi = np.zeros((n, self._tx_L), dtype=np.uint8)
        self.lib.nbl_read_transmitted.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.nbl_read_transmitted(self.h, slot, b0, n, msg.ctypes.data, cw.ctypes.data, txi.ctypes.data))
        return msg, cw, txi

    def read_slot_rx(self, slot, b0, n):
        """diagnostic: the received samples [n][L][2] a slot holds"""
        rx = np.zeros((n, self._tx_L, 2))
        self.lib.nbl_debug_read_slot_rx.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        self._chk(self.lib.nbl_debug_read_slot_rx(self.h, slot, b0, n, rx.ctypes.data))
        return rx

    def set_decoded(self, slot, sym):
        """diagnostic: put decoded words [B][N] where nbl_decode_batch_resident leaves a slot's outputs"""
        sym = np.ascontiguousarray(sym, dtype=np.int32)
        self.lib.nbl_debug_set_decoded.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        self._chk(self.lib.nbl_debug_set_decoded(self.h, slot, sym.ctypes.data, sym.shape[0]))

    def count_errors(self, slot, B):
        es = np.zeros(B, dtype=np.int32)
        eb = np.zeros(B, dtype=np.int32)
        ok = np.zeros(B, dtype=np.uint8)
        self.lib.nbl_count_errors.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.nbl_count_errors(self.h, slot, B, es.ctypes.data, eb.ctypes.data, ok.ctypes.data))
        return es, eb, ok

    def encode_batch(self, msg):
        msg = np.ascontiguousarray(msg, dtype=np.int32)
        B = msg.shape[0]
        cw = np.zeros((B, self.code.N), dtype=np.int32)
        mo = np.zeros_like(msg)
        self.lib.nbl_encode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self._chk(self.lib.nbl_encode_batch(self.h, msg.ctypes.data, B, cw.ctypes.data, mo.ctypes.data))
        return cw, mo

    def channel(self, tx_index, lane_state, sigma):
        """diagnostic: the received samples [B][L][2] the device-side channel forms, and the fraction of log / cos values the host's libm settled"""
        tx_index = np.ascontiguousarray(tx_index, dtype=np.uint8)
        lane_state = np.ascontiguousarray(lane_state, dtype=np.uint32)
        B, L = tx_index.shape
        rx = np.zeros((B, L, 2))
        frac = C.c_double(0)
        self.lib.nbl_debug_channel.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]
        self._chk(self.lib.nbl_debug_channel(self.h, tx_index.ctypes.data, lane_state.ctypes.data, sigma, B, rx.ctypes.data, C.byref(frac)))
        return rx, frac.value

    def debug_osd_sums(self, b):
        """diagnostic: the flag-0 posterior sums S [N][p] of codeword b after the last decode"""
        S = np.zeros((self.code.N, self.code.q.bit_length() - 1))
        self.lib.nbl_debug_osd_sums.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        self._chk(self.lib.nbl_debug_osd_sums(self.h, b, S.ctypes.data))
        return S

    def read_lch(self, b):
        L = np.zeros((self.code.N, self.code.q - 1))
        self.lib.nbl_debug_read_lch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        self._chk(self.lib.nbl_debug_read_lch(self.h, b, L.ctypes.data))
        return L

    def record_state(self, on=True):
        self._chk(self.lib.nbl_set_record_state(self.h, int(on)))

    def defer_last(self, on=True):
        """diagnostic (nbl_debug_defer_last): False = every decode runs the check-node pass of its last iteration itself; True (the
        default) = undamped fused EMS leaves it to the first read of the message state"""
        self.lib.nbl_debug_defer_last.argtypes = [C.c_void_p, C.c_int32]
        self._chk(self.lib.nbl_debug_defer_last(self.h, int(on)))

    def profiling(self, on=True):
        self._chk(self.lib.nbl_set_profiling(self.h, int(on)))

    def last_timing(self):
        ms = (C.c_double * 4)()
        ln = (C.c_int64 * 3)()
        self._chk(self.lib.nbl_last_timing(self.h, ms, ln))
        return list(ms), list(ln)

    def read_state(self, b, post=True, v2c=True):
        """(post, v2c, c2v) of codeword b; post=False / v2c=False pass NULL and return None in that place (a layered EMS decoder has no v2c)"""
        w, N, E = self.code.q - 1, self.code.N, self.code.E
        P = np.zeros((N, w)) if post else None
        V = np.zeros((E, w)) if v2c else None
        Cc = np.zeros((E, w))
        self._chk(self.lib.nbl_read_state(self.h, b, P.ctypes.data if post else None, V.ctypes.data if v2c else None, Cc.ctypes.data))
        return P, V, Cc

    def workspace_bytes(self):
        return self.lib.nbl_workspace_bytes(self.h)
