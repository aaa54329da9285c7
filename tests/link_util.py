"""The link chain of a profile for the GPU tests: work directory, the geometry CComm::Initial derives, and a decoder with demodulator
and transmitter set.  A shipped code and constellation by name (tests/test_gpu_transmitter.py), or a graph spec and a point table
(tests/test_gpu_link_shapes.py)."""
import ctypes as C
import os

import numpy as np

from conftest import decoder_kwargs
import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
from nbldpc_amd import hostlib


def write_points_file(points, path):
    """A point table [order][2] in the reference's constellation file format (nbldpc_amd/datafiles.py::write_constellation_file)."""
    with open(path, "w") as f:
        f.write("\n".join(f"Point:\t{i}\tReal:\t{float(re)!r}\tImag:\t{float(im)!r}" for i, (re, im) in enumerate(points)))
    return path


def prepare_spec_workdir(path, profile_kwargs, spec, points, absolute=False, poly=None):
    """hostlib.prepare_workdir for a graph spec and a point table: SRC/ with the GF tables, code.txt, constellation.txt and
    NBLDPC.Profile.txt.  absolute: the profile names the two files by their full paths.  poly: the modulus of the GF tables (None:
    the default one)."""
    from degree_util import write_spec_code_file
    from nbldpc_amd.profiles import profile_text
    os.makedirs(path, exist_ok=True)
    df.write_gf_tables(spec["q"], os.path.join(path, "SRC"), poly)
    write_spec_code_file(spec, os.path.join(path, "code.txt"))
    write_points_file(points, os.path.join(path, "constellation.txt"))
    kw = dict(profile_kwargs)
    kw["code"] = os.path.join(path, "code.txt") if absolute else "code.txt"
    kw["constellation"] = os.path.join(path, "constellation.txt") if absolute else "constellation.txt"
    prof = os.path.join(path, "NBLDPC.Profile.txt")
    with open(prof, "w") as f:
        f.write(profile_text(**kw))
    return prof


class Link:
    """Work directory of a profile, the geometry CComm::Initial derives from it, and a decoder with demodulator and transmitter set.
    spec / points: a graph spec (tests/degree_util.py) and a constellation table in place of the shipped code_name / cons.  poly: the
    modulus of the field -- the tables of the work directory (from which the host encoder derives `gen`) and those handed to
    nbl_create are made from it."""

    def __init__(self, tmp_path, profile, code_name, cons, P, max_batch=0, with_tx=True, spec=None, points=None, poly=None):
        from nbldpc_amd.profiles import DEFAULTS
        self.dir = str(tmp_path)
        self.prof = dict(DEFAULTS)
        self.prof.update(profile)
        self.prof["parallel"] = P
        kw = {k: v for k, v in self.prof.items() if k not in ("code", "constellation")}
        if spec is None:
            hostlib.prepare_workdir(self.dir, dict(kw, code=code_name), code_name, cons)
            c = df.codes()[code_name]
            self.points = np.array([[x[1], x[2]] for x in sorted(df.constellations()[cons])])
            self.code = nb.Code(code_name)
        else:
            prepare_spec_workdir(self.dir, kw, spec, points, poly=poly)
            c = spec
            self.points = np.ascontiguousarray(points, dtype=np.float64)
            self.code = nb.Code(spec=spec)
        self.c, self.P = c, P
        self.N, self.M, self.q = c["N"], c["M"], c["q"]
        self.K, self.p = self.N - self.M, self.q.bit_length() - 1
        pd = self.prof["puncture_degree"]
        self.punct = [n for n, r in enumerate(c["var_rows"]) if len(r) == pd]
        self.order = self.prof["nqam"]
        mb = self.order.bit_length() - 1
        self.L = (self.N - len(self.punct)) * self.p // mb
        # the index bookkeeping of Demodulate: which sample carries each code bit (BPSK) / code symbol (q-ary), -1 = punctured
        src, k = [], 0
        for n in range(self.N):
            keep = n not in self.punct
            for _ in range(self.p if self.order == 2 else 1):
                src.append(k if keep else -1)
                k += keep
        self.src = np.array(src, dtype=np.int32)
        assert poly is None or spec is not None
        self.gf = None if poly is None else tuple(np.array(t, dtype=np.int64) for t in df.gf_tables(self.q, poly))
        self.dec = nb.Decoder(self.code, self.prof["method"], self.prof["max_iter"], max_batch=max_batch, poll_every=2, gf=self.gf,
                              **decoder_kwargs(self.prof))
        self.dec.set_demodulator(self.order, self.L, self.src, self.points)
        self.gen = hostlib.generator(self.dir, self.N, self.K) if self.prof["random_msg"] else None
        if with_tx:
            self.set_tx()
        self.lib = nb.load_library()
        self.lib.nbl_rand_advance.argtypes = [C.c_void_p, C.c_uint64]
        self.lib.nbl_rand_advance.restype = None

    def set_tx(self, **over):
        a = dict(gen=self.gen, crc_len=self.prof["crc_len"], random_msg=self.prof["random_msg"], parallel=self.P, punct=self.punct,
                 mod_order=self.order, n_mod_sym=self.L)
        a.update(over)
        self.dec.set_transmitter(**a)

    def states(self, frames, state0):
        """per frame: PN register [P] and generator state [P][3] of every lane, moved on with the two helpers of the ABI"""
        clocks = (self.K * self.p - self.prof["crc_len"]) * self.P if self.prof["random_msg"] else 0
        pn = np.array([hostlib.pn_initial(i) for i in range(self.P)], dtype=np.uint16)
        st = np.ascontiguousarray(state0, dtype=np.uint32).copy()
        out = []
        for _ in range(frames):
            out.append((pn.copy(), st.copy()))
            pn = np.array([hostlib.pn_advance(int(s), clocks) for s in pn], dtype=np.uint16)
            for i in range(self.P):
                self.lib.nbl_rand_advance(st[i].ctypes.data, 4 * self.L)
        return out

    def host_chain(self, ebn0, frames):
        """the host chain's frames, b = frame * P + lane: tx_code, tx_msg, rx, tx_index, generator states, sigma"""
        _, tx, msg, sigma = hostlib.frontend(self.dir, ebn0, frames, self.N, self.K, self.q, self.P)
        rx, txi, state, sigma2 = hostlib.channel(self.dir, ebn0, frames, self.L, self.P)
        assert sigma == sigma2
        return tx, msg, rx, txi, state, sigma

    def check_chain(self, ebn0, frames, want_code=None, want_msg=None):
        P = self.P
        tx, msg, rx, txi, state, sigma = self.host_chain(ebn0, frames)
        if want_code is not None:   # the compiled reference's own arrays
            assert np.array_equal(tx, want_code) and np.array_equal(msg, want_msg)
        for f, (pn, st) in enumerate(self.states(frames, state[:P])):
            assert np.array_equal(st, state[f * P:(f + 1) * P]), f   # nbl_rand_advance follows the host chain's generators
            slot = f & 1
            self.dec.transmit_batch(slot, pn, st, sigma)
            m, cw, ti = self.dec.read_transmitted(slot, 0, P)
            sl = slice(f * P, (f + 1) * P)
            assert np.array_equal(cw, tx[sl]), ("tx_code", f)
            assert np.array_equal(m, msg[sl]), ("tx_msg", f)
            assert np.array_equal(ti, txi[sl]), ("tx_index", f)
            got = self.dec.read_slot_rx(slot, 0, P)
            assert np.array_equal(got.view(np.uint64), rx[sl].view(np.uint64)), ("rx", f)
        return tx, msg, sigma
