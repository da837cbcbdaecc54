"""ctypes bindings of the device-primitive probe (tests/probes/b9_prims_probe.hip -> build/probes/libb9prims.so): every
call hands numpy arrays to one kernel that only applies a shipped device function to them.  `Prims` binds ANY library with
the probe's entry points -- tests/test_prims_host.py binds the CPU emulation (tests/probes/b9_prims_emul.cpp) through it, so
the checkers of tests/prims_check.py run unchanged on both.

load() rebuilds the library when it is older than its sources and hipcc is present; a missing library with no compiler is
an error (a test FAILURE, never a skip)."""
import ctypes
import os
import shutil

import numpy as np

from base_amd import build

M1 = dict(log_ge1=0, log_pos=1, exp_fast=2, log1pexp=3, exp10=4, log10=5)      # 4, 5: the library's, as wd_chain calls them
M2 = dict(logaddexp=0, fdiv=1, mix_value=2)
SEARCH = dict(bracket=0, bracket8=1, bracket8_desc=2, find_bracket=3)
WAVE1 = dict(wave_sum=0, wave_max_all=1, wave_bcast0=2, wave_uniform=3)

_P = ctypes.c_void_p


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(_P)


def mass_column_capacity(n: int) -> int:
    """Doubles a mass column of n nodes occupies where find_bracket searches it.  The staging code (k_star_like, heavy_stars,
    b9_kernels.hip's LDS sizes) keeps a column in mass_cap = (max_eep + 1) & ~1 >= n doubles and ALWAYS has 8 more readable
    doubles behind them (the next column, the magnitude rows, or the `+ 8` of the LDS size), so the tail probe's reads at
    lo + 1 .. lo + 7 <= n + 5 stay inside: the tightest case, n == max_eep, is restated here."""
    return ((n + 1) & ~1) + 8


class Prims:
    def __init__(self, path: str):
        self.path = path
        self.lib = ctypes.CDLL(path)
        for name in ("b9p_map1", "b9p_map2", "b9p_u01", "b9p_philox", "b9p_search", "b9p_lockstep2", "b9p_lane_down_f64",
                     "b9p_lane_down_i32", "b9p_wave1", "b9p_wave_sum7", "b9p_mix", "b9p_lse", "b9p_box_store", "b9p_box_bound"):
            getattr(self.lib, name).restype = ctypes.c_int

    @staticmethod
    def _ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: status {rc}")

    def map1(self, op, x):
        x = _f64(x); y = np.empty_like(x)
        self._ok(self.lib.b9p_map1(ctypes.c_int(M1[op]), _ptr(x), _ptr(y), ctypes.c_longlong(x.size)), op)
        return y

    def map2(self, op, a, b):
        a, b = np.broadcast_arrays(_f64(a), _f64(b))
        a, b = _f64(a), _f64(b); y = np.empty_like(a)
        self._ok(self.lib.b9p_map2(ctypes.c_int(M2[op]), _ptr(a), _ptr(b), _ptr(y), ctypes.c_longlong(a.size)), op)
        return y

    def u01(self, hi, lo):
        hi = np.ascontiguousarray(hi, dtype=np.uint32); lo = np.ascontiguousarray(lo, dtype=np.uint32)
        u = np.empty(hi.size); lg = np.empty(hi.size)
        self._ok(self.lib.b9p_u01(_ptr(hi), _ptr(lo), _ptr(u), _ptr(lg), ctypes.c_longlong(hi.size)), "u01")
        return u, lg

    def philox(self, ctr, key):
        ctr = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4); key = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2)
        assert len(ctr) == len(key)
        out = np.empty_like(ctr)
        self._ok(self.lib.b9p_philox(_ptr(ctr), _ptr(key), _ptr(out), ctypes.c_longlong(len(ctr))), "philox")
        return out

    def search(self, op, column, n, x, lds=False):
        """column: the n nodes followed by the caller's padding.  -> (index, t) per query (t: find_bracket only, else 0)"""
        column = _f64(column); x = _f64(x)
        lo = np.empty(x.size, dtype=np.int32); t = np.empty(x.size)
        self._ok(self.lib.b9p_search(ctypes.c_int(SEARCH[op]), ctypes.c_int(int(lds)), _ptr(column), ctypes.c_int(n), ctypes.c_int(column.size),
                                     _ptr(x), _ptr(lo), _ptr(t), ctypes.c_longlong(x.size)), op)
        return lo, t

    def lockstep2(self, a0, a1, x):
        a0, a1, x = _f64(a0), _f64(a1), _f64(x)
        l0 = np.empty(x.size, dtype=np.int32); l1 = np.empty(x.size, dtype=np.int32)
        self._ok(self.lib.b9p_lockstep2(_ptr(a0), ctypes.c_int(a0.size), _ptr(a1), ctypes.c_int(a1.size), _ptr(x), _ptr(l0), _ptr(l1),
                                        ctypes.c_longlong(x.size)), "lockstep2")
        return l0, l1

    def lane_down(self, O, v):
        """v: [waves][64] float64 or int32"""
        if np.asarray(v).dtype == np.int32:
            v = np.ascontiguousarray(v); out = np.empty_like(v)
            self._ok(self.lib.b9p_lane_down_i32(ctypes.c_int(O), _ptr(v), _ptr(out), ctypes.c_int(v.shape[0])), "lane_down<int>")
        else:
            v = _f64(v); out = np.empty_like(v)
            self._ok(self.lib.b9p_lane_down_f64(ctypes.c_int(O), _ptr(v), _ptr(out), ctypes.c_int(v.shape[0])), "lane_down<double>")
        return out

    def wave1(self, op, v):
        v = _f64(v); assert v.ndim == 2 and v.shape[1] == 64
        out = np.empty_like(v)
        self._ok(self.lib.b9p_wave1(ctypes.c_int(WAVE1[op]), _ptr(v), _ptr(out), ctypes.c_int(v.shape[0])), op)
        return out

    def wave_sum7(self, v):
        v = _f64(v); assert v.ndim == 3 and v.shape[1:] == (7, 64)
        out = np.empty_like(v)
        self._ok(self.lib.b9p_wave_sum7(_ptr(v), _ptr(out), ctypes.c_int(v.shape[0])), "wave_sum7")
        return out

    def mix(self, ea, l):
        """ea, l: [waves][k][64] -> mix_wave_total of each wave"""
        ea, l = _f64(ea), _f64(l); assert ea.shape == l.shape and ea.ndim == 3 and ea.shape[2] == 64
        tot = np.empty(ea.shape[0])
        self._ok(self.lib.b9p_mix(_ptr(ea), _ptr(l), ctypes.c_int(ea.shape[1]), _ptr(tot), ctypes.c_int(ea.shape[0])), "mix")
        return tot

    def lse(self, terms, parts=1):
        """terms: [sequences][terms], dealt in contiguous runs over `parts` accumulators merged in a tree -> (mx, sm)"""
        terms = _f64(terms); assert terms.ndim == 2
        mx = np.empty(terms.shape[0]); sm = np.empty(terms.shape[0])
        self._ok(self.lib.b9p_lse(_ptr(terms), ctypes.c_int(terms.shape[0]), ctypes.c_int(terms.shape[1]), ctypes.c_int(parts), _ptr(mx), _ptr(sm)), "lse")
        return mx, sm

    def box_store(self, lo, hi):
        """lo, hi: [boxes][nfp] -> box [boxes][2][nfp] float64, box_f [boxes][2][nfp] float32"""
        lo, hi = _f64(lo), _f64(hi); nb, nfp = lo.shape
        box = np.empty((nb, 2, nfp)); box_f = np.empty((nb, 2, nfp), dtype=np.float32)
        self._ok(self.lib.b9p_box_store(ctypes.c_int(nfp), _ptr(lo), _ptr(hi), _ptr(box), _ptr(box_f), ctypes.c_longlong(nb)), "box_store")
        return box, box_f

    def box_bound(self, so, sw, box, box_f, nbm, xcut):
        """so, sw: [boxes][64][nfp] -> dict(lb64, lb32, slack: [boxes][64]; pass64, pass32: [boxes])"""
        so, sw, box, nbm, xcut = _f64(so), _f64(sw), _f64(box), _f64(nbm), _f64(xcut)
        box_f = np.ascontiguousarray(box_f, dtype=np.float32)
        nb, _, nfp = so.shape
        assert so.shape == sw.shape == (nb, 64, nfp) and box.shape == box_f.shape == (nb, 2, nfp) and nbm.shape == xcut.shape == (nb,)
        r = dict(lb64=np.empty((nb, 64)), lb32=np.empty((nb, 64)), slack=np.empty((nb, 64)),
                 pass64=np.empty(nb, dtype=np.int32), pass32=np.empty(nb, dtype=np.int32))
        self._ok(self.lib.b9p_box_bound(ctypes.c_int(nfp), _ptr(so), _ptr(sw), _ptr(box), _ptr(box_f), _ptr(nbm), _ptr(xcut), _ptr(r["lb64"]),
                                        _ptr(r["lb32"]), _ptr(r["slack"]), _ptr(r["pass64"]), _ptr(r["pass32"]), ctypes.c_longlong(nb)), "box_bound")
        return r


_probe = None


def load() -> Prims:
    """The probe on the GPU.  Stale or missing + a compiler: rebuilt.  Missing + no compiler: an error."""
    global _probe
    if _probe is None:
        have_cc = shutil.which("hipcc") is not None or os.path.exists(build.HIPCC)
        if have_cc:
            build.build_probe()
        elif not os.path.exists(build.PROBE_LIB):
            raise RuntimeError(f"{build.PROBE_LIB} is missing and there is no hipcc to build it: run __graft_entry__.build() where the compiler is")
        _probe = Prims(build.PROBE_LIB)
    return _probe
