"""ctypes binding of libbase9host.so (include/base9_host.h): the C++ walker-parallel sampler and its exchanges.

Plumbing only.  `HostSampler` drives the C++ `b9h::WalkerSampler` -- on the GPU through a `b9_ctx` (the product path:
device-resident blocks, summary rows condensed on the device, RCCL all-gather from HBM), or, for tests of the C++ host
logic on a machine without a GPU, through caller-supplied callbacks (block runner, evaluator, all-gather).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Optional, Sequence

import numpy as np

from . import abi

HOST_DIR = os.path.join(abi.REPO_ROOT, "base_amd", "host")
HOST_LIB_PATH = os.path.join(HOST_DIR, "libbase9host.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
vp = C.c_void_p

GATHER_FN = C.CFUNCTYPE(C.c_int, vp, _dp, C.c_size_t, _dp)
BLOCK_FN = C.CFUNCTYPE(C.c_int, vp, _dp, _dp, _ip, C.c_int, _ip, C.c_int, _dp, C.c_uint64, C.c_int64, C.c_int,
                       _dp, _dp, _dp, _dp, C.POINTER(C.c_int64))
LOGPOST_FN = C.CFUNCTYPE(C.c_int, vp, _dp, C.c_int, _dp)

#: every function include/base9_host.h declares (checked by tests/test_abi.py against the header)
HOST_SYMBOLS = [
    "b9h_last_error", "b9h_rank_from_env", "b9h_device_synchronize",
    "b9h_exchange_local", "b9h_exchange_rccl", "b9h_exchange_callback", "b9h_exchange_free", "b9h_exchange_barrier",
    "b9h_exchange_max", "b9h_exchange_world", "b9h_exchange_name", "b9h_exchange_comm_ranks", "b9h_exchange_devices",
    "b9h_group_check", "b9h_forced_ranks", "b9h_test_stall",
    "b9h_sampler_create", "b9h_sampler_create_callback", "b9h_sampler_free", "b9h_sampler_initialise", "b9h_sampler_run",
    "b9h_sampler_n_local", "b9h_sampler_state", "b9h_summary_rows",
    "b9h_load_pack", "b9h_free_pack", "b9h_read_phot", "b9h_free_phot", "b9h_settings_dump", "b9h_merge_parts",
    "b9h_sim_draw_systems", "b9h_sim_field_mags", "b9h_scatter", "b9h_sim_settings", "b9h_read_res_rows",
    "b9h_star_table", "b9h_write_star_summary", "b9h_wd_table", "b9h_write_wd_summary",
    "b9h_mass_function_table", "b9h_write_mass_function", "b9h_write_star_mass_hist", "b9h_mass_function_settings",
    "b9h_binary_table", "b9h_ratio_dist_table", "b9h_star_ratio_table", "b9h_write_binary_fraction", "b9h_write_ratio_dist", "b9h_write_star_ratio",
    "b9h_refine_star_edges", "b9h_star_intervals_table", "b9h_write_star_intervals", "b9h_star_intervals_settings",
    "b9h_wd_first_ranges", "b9h_wd_intervals_table", "b9h_write_wd_intervals", "b9h_wd_intervals_settings",
    "b9h_band_first_ranges", "b9h_band_first_edges", "b9h_band_table", "b9h_write_cmd_band", "b9h_cmd_band_settings",
    "b9h_resid_table", "b9h_filter_resid_table", "b9h_write_phot_resid", "b9h_write_filter_resid", "b9h_phot_resid_settings",
    "b9h_loo_table", "b9h_filter_loo_table", "b9h_write_star_filter_check", "b9h_write_filter_check", "b9h_filter_check_settings",
    "b9h_offset_direction", "b9h_offset_table", "b9h_offset_dist_table", "b9h_write_star_offsets", "b9h_write_offset_dist", "b9h_star_offsets_settings",
    "b9h_pointwise_table", "b9h_score_totals", "b9h_score_compare", "b9h_write_pointwise", "b9h_write_model_score", "b9h_model_score_settings",
    "b9h_influence_table", "b9h_group_influence_table", "b9h_influence_quantities", "b9h_influence_groups", "b9h_write_star_influence",
    "b9h_write_group_influence", "b9h_star_influence_settings",
]

_lib = None


def load() -> C.CDLL:
    """dlopen libbase9host.so (which pulls in libbase9hip.so, librccl and libamdhip64) and declare its prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(HOST_LIB_PATH):
        raise RuntimeError(f"{HOST_LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(HOST_LIB_PATH)
    lib.b9h_last_error.restype = C.c_char_p
    lib.b9h_rank_from_env.argtypes = [C.POINTER(C.c_int)] * 3
    lib.b9h_rank_from_env.restype = None
    lib.b9h_exchange_local.argtypes = [C.POINTER(vp)]
    lib.b9h_exchange_rccl.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(vp)]
    lib.b9h_exchange_callback.argtypes = [GATHER_FN, vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.b9h_exchange_free.argtypes = [vp]
    lib.b9h_exchange_free.restype = None
    lib.b9h_exchange_barrier.argtypes = [vp]
    lib.b9h_exchange_max.argtypes = [vp, C.c_double, _dp]
    lib.b9h_exchange_world.argtypes = [vp]
    lib.b9h_exchange_name.argtypes = [vp]
    lib.b9h_exchange_name.restype = C.c_char_p
    lib.b9h_exchange_comm_ranks.argtypes = [vp]
    lib.b9h_exchange_devices.argtypes = [vp, C.c_char_p, C.c_int]
    lib.b9h_test_stall.argtypes = [C.c_char_p, C.c_int]
    lib.b9h_group_check.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    lib.b9h_test_stall.restype = None
    lib.b9h_sampler_create.argtypes = [vp, C.c_int, C.c_int, _ip, _dp, C.c_int, C.c_uint64, C.c_int, vp, C.POINTER(vp)]
    lib.b9h_sampler_create_callback.argtypes = [BLOCK_FN, LOGPOST_FN, vp, C.c_int, _ip, _dp, C.c_int, C.c_uint64, C.c_int, vp, C.POINTER(vp)]
    lib.b9h_sampler_free.argtypes = [vp]
    lib.b9h_sampler_free.restype = None
    lib.b9h_sampler_initialise.argtypes = [vp, _dp]
    lib.b9h_sampler_run.argtypes = [vp, C.c_int64, C.c_int, _dp, _dp]
    lib.b9h_sampler_n_local.argtypes = [vp]
    lib.b9h_sampler_state.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _dp, _dp, _dp, _dp]
    lib.b9h_summary_rows.argtypes = [_dp, _dp, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp]
    lib.b9h_load_pack.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(vp), C.POINTER(abi.b9_pack)]
    lib.b9h_free_pack.argtypes = [vp]
    lib.b9h_read_phot.argtypes = [C.c_char_p, C.c_double, C.c_double, C.c_int, C.POINTER(vp), C.POINTER(abi.b9_stars), C.c_char_p, C.c_int]
    lib.b9h_free_phot.argtypes = [vp]
    lib.b9h_settings_dump.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    lib.b9h_merge_parts.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_long]
    lib.b9h_read_res_rows.argtypes = [C.c_char_p, _dp, C.c_int, _dp, C.c_long, C.POINTER(C.c_long)]
    lib.b9h_star_table.argtypes = [_dp, C.c_long, _dp]
    lib.b9h_write_star_summary.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, _dp, C.c_int]
    lib.b9h_wd_table.argtypes = [_dp, C.c_long, _dp]
    lib.b9h_write_wd_summary.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, _dp, C.c_int]
    lib.b9h_mass_function_table.argtypes = [_dp, C.c_long, _dp, C.c_int, _dp]
    lib.b9h_write_mass_function.argtypes = [C.c_char_p, _dp, C.c_int]
    lib.b9h_write_star_mass_hist.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, _dp, C.c_int, C.c_long]
    lib.b9h_mass_function_settings.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_double, C.c_char_p, C.c_int, _dp]
    lib.b9h_binary_table.argtypes = [_dp, C.c_long, _dp, C.c_int, C.c_int, C.c_double, _dp]
    lib.b9h_ratio_dist_table.argtypes = [_dp, C.c_long, C.c_int, C.c_int, _dp]
    lib.b9h_star_ratio_table.argtypes = [_dp, C.c_long, C.c_int, C.c_int, C.c_double, C.c_long, _dp]
    lib.b9h_write_binary_fraction.argtypes = [C.c_char_p, _dp, C.c_int]
    lib.b9h_write_ratio_dist.argtypes = [C.c_char_p, _dp, C.c_int, C.c_int]
    lib.b9h_write_star_ratio.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, _dp, C.c_int]
    lib.b9h_refine_star_edges.argtypes = [_dp, _dp, C.c_long, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp]
    lib.b9h_star_intervals_table.argtypes = [C.c_long, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, _dp]
    lib.b9h_write_star_intervals.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, _dp, C.c_int, _dp]
    lib.b9h_star_intervals_settings.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    lib.b9h_wd_first_ranges.argtypes = [_dp, C.c_long, C.c_int, _dp, _dp]
    lib.b9h_wd_intervals_table.argtypes = [C.c_long, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp]
    lib.b9h_write_wd_intervals.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, C.c_int, _dp, C.c_int, _dp]
    lib.b9h_wd_intervals_settings.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    lib.b9h_band_first_ranges.argtypes = [_dp, C.c_long, _dp, _dp]
    lib.b9h_band_first_edges.argtypes = [_dp, C.c_long, C.c_int, _dp]
    lib.b9h_band_table.argtypes = [_dp, _dp, C.c_long, C.c_int, _dp, _dp, _dp, _ip, _ip, _dp]
    lib.b9h_write_cmd_band.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, _dp, C.c_int, _dp]
    lib.b9h_cmd_band_settings.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    lib.b9h_resid_table.argtypes = [_dp, _dp, _dp, C.c_long, C.c_int, _dp]
    lib.b9h_filter_resid_table.argtypes = [_dp, C.c_long, C.c_int, _dp]
    lib.b9h_write_phot_resid.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, C.POINTER(C.c_char_p), C.c_int, _dp]
    lib.b9h_write_filter_resid.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, _dp]
    lib.b9h_phot_resid_settings.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    lib.b9h_loo_table.argtypes = [_dp, _dp, _dp, C.c_long, C.c_int, _dp]
    lib.b9h_filter_loo_table.argtypes = [_dp, C.c_long, C.c_int, _dp]
    lib.b9h_write_star_filter_check.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, C.POINTER(C.c_char_p), C.c_int, _dp]
    lib.b9h_write_filter_check.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, _dp]
    lib.b9h_filter_check_settings.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    lib.b9h_offset_direction.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, _dp, _dp]
    lib.b9h_offset_table.argtypes = [_dp, _dp, _dp, _dp, C.c_long, C.c_int, C.c_int, _dp]
    lib.b9h_offset_dist_table.argtypes = [_dp, C.c_long, C.c_int, _dp]
    lib.b9h_write_star_offsets.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, C.POINTER(C.c_char_p), C.c_int, _dp]
    lib.b9h_write_offset_dist.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, _dp]
    lib.b9h_star_offsets_settings.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    lib.b9h_pointwise_table.argtypes = [_dp, _dp, C.c_int, C.c_long, _dp]
    lib.b9h_score_totals.argtypes = [_dp, C.c_long, _dp]
    lib.b9h_score_compare.argtypes = [_dp, C.POINTER(C.c_char_p), C.c_long, _dp, C.POINTER(C.c_char_p), C.c_long, _dp]
    lib.b9h_write_pointwise.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, _dp]
    lib.b9h_write_model_score.argtypes = [C.c_char_p, _dp]
    lib.b9h_model_score_settings.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    lib.b9h_influence_table.argtypes = [_dp, _dp, C.c_int, C.c_long, C.c_int, _dp]
    lib.b9h_group_influence_table.argtypes = [_dp, C.c_long, C.c_int, _dp, C.c_int, _ip, C.c_long, _dp]
    lib.b9h_influence_quantities.argtypes = [C.c_int, C.POINTER(C.c_char_p), _dp, _dp, C.c_long, C.c_char_p, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int)]
    lib.b9h_influence_groups.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), _ip, C.c_long, C.c_char_p, C.c_int, _ip, C.POINTER(C.c_int)]
    lib.b9h_write_star_influence.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_long, C.POINTER(C.c_char_p), C.c_int, _dp]
    lib.b9h_write_group_influence.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.c_int, _dp]
    lib.b9h_star_influence_settings.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    lib.b9h_sim_draw_systems.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                         C.c_int, C.c_double, _dp, _dp, _dp, _ip, _ip]
    lib.b9h_sim_field_mags.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int, _dp, _dp, _dp]
    lib.b9h_scatter.argtypes = [C.c_uint64, C.POINTER(C.c_int64), C.c_int64, C.c_int, _dp, C.c_double, C.c_double, C.c_double, _dp, _dp]
    lib.b9h_sim_settings.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    _lib = lib
    return lib


class HostError(RuntimeError):
    pass


def _check(rc: int) -> None:
    if rc != 0:
        raise HostError(load().b9h_last_error().decode())


def rank_from_env():
    r, w, l = C.c_int(0), C.c_int(1), C.c_int(0)
    load().b9h_rank_from_env(C.byref(r), C.byref(w), C.byref(l))
    return r.value, w.value, l.value


class Exchange:
    """How the walkers' block summary rows travel between ranks."""

    def __init__(self, handle: vp, keep=None):
        self._h, self._keep = handle, keep

    @classmethod
    def local(cls) -> "Exchange":
        h = vp()
        _check(load().b9h_exchange_local(C.byref(h)))
        return cls(h)

    @classmethod
    def rccl(cls, rank: int, world: int, device: int, directory: Optional[str] = None) -> "Exchange":
        """One process per GPU; the RCCL unique id travels through a file (b9dist.hpp)."""
        h = vp()
        _check(load().b9h_exchange_rccl(rank, world, directory.encode() if directory else None, device, C.byref(h)))
        return cls(h)

    @classmethod
    def callback(cls, all_gather: Callable[[np.ndarray], np.ndarray], rank: int, world: int) -> "Exchange":
        """Test seam: `all_gather(rows[count]) -> rows[world * count]` (e.g. gloo through torch.distributed)."""
        def _gather(_user, mine, count, out):
            try:
                got = np.asarray(all_gather(np.ctypeslib.as_array(mine, shape=(count,)).copy()), dtype=np.float64).ravel()
                np.ctypeslib.as_array(out, shape=(count * world,))[:] = got
                return 0
            except Exception:      # noqa: BLE001 -- reported through the C return code
                import traceback
                traceback.print_exc()
                return 1
        fn = GATHER_FN(_gather)
        h = vp()
        _check(load().b9h_exchange_callback(fn, None, rank, world, C.byref(h)))
        return cls(h, keep=fn)

    def barrier(self) -> None:
        _check(load().b9h_exchange_barrier(self._h))

    def max(self, value: float) -> float:
        out = C.c_double(0)
        _check(load().b9h_exchange_max(self._h, float(value), C.byref(out)))
        return out.value

    @property
    def world(self) -> int:
        return int(load().b9h_exchange_world(self._h))

    @property
    def name(self) -> str:
        return load().b9h_exchange_name(self._h).decode()

    @property
    def comm_ranks(self) -> int:
        """ncclCommCount of the exchange's communicator (0: it has none)."""
        return int(load().b9h_exchange_comm_ranks(self._h))

    @property
    def devices(self):
        """PCI bus ids of the ranks' GPUs in rank order, gathered through the communicator ([] without one)."""
        buf = C.create_string_buffer(4096)
        if load().b9h_exchange_devices(self._h, buf, len(buf)) != 0:
            raise HostError("b9h_exchange_devices: buffer too small")
        txt = buf.value.decode()
        return txt.split(",") if txt else []

    def close(self) -> None:
        if self._h:
            load().b9h_exchange_free(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:     # noqa: BLE001
            pass


class HostSampler:
    """b9h::WalkerSampler.  `engine` = a base_amd.engine.Engine (GPU), or runner callbacks for the CPU test seam."""

    def __init__(self, n_walkers: int, free: Sequence[int], step: Sequence[float], exchange: Exchange, seed: int = 1234,
                 block: int = 50, engine=None, run_block: Optional[Callable] = None, evaluate: Optional[Callable] = None):
        lib = load()
        self.exchange = exchange
        self.free = np.ascontiguousarray(free, dtype=np.int32)
        self.d = len(self.free)
        self.n_walkers = int(n_walkers)
        stepv = np.ascontiguousarray(step, dtype=np.float64)
        self._h = vp()
        self._keep = []
        if engine is not None:
            self._keep.append(engine)
            _check(lib.b9h_sampler_create(engine._ctx, int(engine.options.mode), self.n_walkers, self.free.ctypes.data_as(_ip),
                                          stepv.ctypes.data_as(_dp), self.d, int(seed), int(block), exchange._h, C.byref(self._h)))
        else:
            d = self.d

            def _run(_u, p_in, lp_in, ids, n_local, free_idx, dd, chol, seed_, step0, n_steps, p_out, lp_out, samples, lps, n_acc):
                try:
                    params = np.ctypeslib.as_array(p_in, shape=(n_local, abi.B9_NPARAM)).copy()
                    logpost = np.ctypeslib.as_array(lp_in, shape=(n_local,)).copy()
                    wid = np.ctypeslib.as_array(ids, shape=(n_local,)).copy()
                    fr = np.ctypeslib.as_array(free_idx, shape=(dd,)).astype(np.int64)
                    ch = np.ctypeslib.as_array(chol, shape=(dd, dd)).copy()
                    po, lo, sa, ls, na = run_block(params, logpost, wid, fr, ch, int(seed_), int(step0), int(n_steps))
                    np.ctypeslib.as_array(p_out, shape=(n_local, abi.B9_NPARAM))[:] = po
                    np.ctypeslib.as_array(lp_out, shape=(n_local,))[:] = lo
                    np.ctypeslib.as_array(samples, shape=(n_steps, n_local, dd))[:] = sa
                    np.ctypeslib.as_array(lps, shape=(n_steps, n_local))[:] = ls
                    n_acc[0] = int(na)
                    return 0
                except Exception:      # noqa: BLE001
                    import traceback
                    traceback.print_exc()
                    return 1

            def _eval(_u, params, n, out):
                try:
                    np.ctypeslib.as_array(out, shape=(n,))[:] = evaluate(np.ctypeslib.as_array(params, shape=(n, abi.B9_NPARAM)).copy())
                    return 0
                except Exception:      # noqa: BLE001
                    import traceback
                    traceback.print_exc()
                    return 1

            self._keep += [BLOCK_FN(_run), LOGPOST_FN(_eval)]
            _check(lib.b9h_sampler_create_callback(self._keep[0], self._keep[1], None, self.n_walkers, self.free.ctypes.data_as(_ip),
                                                   stepv.ctypes.data_as(_dp), d, int(seed), int(block), exchange._h, C.byref(self._h)))
        self.n_local = int(lib.b9h_sampler_n_local(self._h))

    def initialise(self, start: np.ndarray) -> None:
        start = np.ascontiguousarray(start, dtype=np.float64).reshape(self.n_walkers, abi.B9_NPARAM)
        _check(load().b9h_sampler_initialise(self._h, start.ctypes.data_as(_dp)))

    def run(self, n_steps: int, adapt: bool = True, record: bool = False):
        """Returns (samples[n_steps, n_local, d], lps[n_steps, n_local]) when `record`, else None."""
        if record:
            samples = np.empty((n_steps, self.n_local, self.d))
            lps = np.empty((n_steps, self.n_local))
            _check(load().b9h_sampler_run(self._h, int(n_steps), int(bool(adapt)), samples.ctypes.data_as(_dp), lps.ctypes.data_as(_dp)))
            return samples, lps
        _check(load().b9h_sampler_run(self._h, int(n_steps), int(bool(adapt)), None, None))
        return None

    def state(self) -> dict:
        steps, acc, scale = C.c_int64(0), C.c_int64(0), C.c_double(0)
        chol = np.empty((self.d, self.d))
        allp = np.empty((self.n_walkers, abi.B9_NPARAM))
        alll = np.empty(self.n_walkers)
        _check(load().b9h_sampler_state(self._h, C.byref(steps), C.byref(acc), C.byref(scale), chol.ctypes.data_as(_dp),
                                        allp.ctypes.data_as(_dp), alll.ctypes.data_as(_dp)))
        return dict(steps=steps.value, accepted_local=acc.value, scale=scale.value, chol=chol, all_params=allp, all_logpost=alll)

    def close(self) -> None:
        if self._h:
            load().b9h_sampler_free(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:     # noqa: BLE001
            pass


def summary_rows(samples: np.ndarray, params_end: np.ndarray, logpost_end: np.ndarray, origin: np.ndarray) -> np.ndarray:
    """b9h::summary_rows: the host statement of the device's block summary rows."""
    samples = np.ascontiguousarray(samples, dtype=np.float64)
    n, wl, d = samples.shape
    pe = np.ascontiguousarray(params_end, dtype=np.float64)
    le = np.ascontiguousarray(logpost_end, dtype=np.float64)
    og = np.ascontiguousarray(origin, dtype=np.float64)
    rows = np.empty((wl, abi.row_doubles(d)))
    _check(load().b9h_summary_rows(samples.ctypes.data_as(_dp), pe.ctypes.data_as(_dp), le.ctypes.data_as(_dp), n, wl, d,
                                   og.ctypes.data_as(_dp), rows.ctypes.data_as(_dp)))
    return rows


def read_res_rows(path: str, start_row, stage: int = 3) -> np.ndarray:
    """b9h_read_res_rows: the rows of a .res whose stage column equals `stage`, as full parameter rows [n, B9_NPARAM]
    (start_row with the file's sampled columns written over it) -- what sampleMass and sampleWDMass read."""
    start = np.ascontiguousarray(start_row, dtype=np.float64).reshape(12)
    n = C.c_long(0)
    _check(load().b9h_read_res_rows(path.encode(), start.ctypes.data_as(_dp), int(stage), None, 0, C.byref(n)))
    rows = np.empty((n.value, 12))
    if n.value:
        _check(load().b9h_read_res_rows(path.encode(), start.ctypes.data_as(_dp), int(stage), rows.ctypes.data_as(_dp), n.value, C.byref(n)))
    return rows


STAR_TABLE_COLUMNS = ("rows", "member", "mass", "massSd", "massRatio", "massRatioSd", "pBinary", "pPop2")


def star_table(acc) -> np.ndarray:
    """b9h_star_table: b9_star_moments' accumulators [n_stars, 8] -> the derived columns [n_stars, 8] (STAR_TABLE_COLUMNS)."""
    acc = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1, 8)
    out = np.empty_like(acc)
    _check(load().b9h_star_table(acc.ctypes.data_as(_dp), acc.shape[0], out.ctypes.data_as(_dp)))
    return out


def write_star_summary(path: str, ids, acc, n_pops: int = 1) -> None:
    """b9h_write_star_summary: the .starSummary file of the accumulators `acc` [len(ids), 8]."""
    acc = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1, 8)
    if acc.shape[0] != len(ids):
        raise ValueError("one id per star")
    arr = (C.c_char_p * len(ids))(*[str(i).encode() for i in ids])
    _check(load().b9h_write_star_summary(path.encode(), arr, len(ids), acc.ctypes.data_as(_dp), int(n_pops)))


def read_star_summary(path: str):
    """(ids, columns, table [n_stars, len(columns)]) of a .starSummary file."""
    with open(path) as f:
        header = f.readline().split()
        if header[:1] != ["id"]:
            raise HostError(path + ": not a .starSummary file")
        ids, rows = [], []
        for line in f:
            t = line.split()
            if not t:
                continue
            if len(t) != len(header):
                raise HostError(path + ": a line does not hold one value per column")
            ids.append(t[0])
            rows.append([float(x) for x in t[1:]])
    return ids, header[1:], np.array(rows, dtype=np.float64).reshape(len(ids), len(header) - 1)


WD_TABLE_COLUMNS = ("rows", "member", "pCooled", "zamsMass", "zamsMassSd", "wdMass", "wdMassSd", "precLogAge", "precLogAgeSd",
                    "logCoolAge", "logCoolAgeSd", "logTeff", "logTeffSd", "logg", "loggSd", "pPop2")


def wd_table(acc) -> np.ndarray:
    """b9h_wd_table: b9_wd_moments' accumulators [n_wd, 16] -> the derived columns [n_wd, 16] (WD_TABLE_COLUMNS)."""
    acc = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1, 16)
    out = np.empty_like(acc)
    _check(load().b9h_wd_table(acc.ctypes.data_as(_dp), acc.shape[0], out.ctypes.data_as(_dp)))
    return out


def write_wd_summary(path: str, ids, acc, n_pops: int = 1) -> None:
    """b9h_write_wd_summary: the .wdSummary file of the accumulators `acc` [len(ids), 16]."""
    acc = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1, 16)
    if acc.shape[0] != len(ids):
        raise ValueError("one id per WD-stage star")
    arr = (C.c_char_p * len(ids))(*[str(i).encode() for i in ids])
    _check(load().b9h_write_wd_summary(path.encode(), arr, len(ids), acc.ctypes.data_as(_dp), int(n_pops)))


def read_wd_summary(path: str):
    """(ids, columns, table [n_wd, len(columns)]) of a .wdSummary file: the layout of a .starSummary file."""
    return read_star_summary(path)


MASS_FUNCTION_COLUMNS = ("lo", "hi", "mean", "sd", "p16", "p50", "p84", "dNdlogM")


def mass_function_table(row_hist, edges) -> np.ndarray:
    """b9h_mass_function_table: b9_mass_hist's row_hist [n_rows, n_bins + 1] -> the per-bin table [n_bins, 8]
    (MASS_FUNCTION_COLUMNS)."""
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    n_bins = len(edges) - 1
    rh = np.ascontiguousarray(row_hist, dtype=np.float64).reshape(-1, n_bins + 1)
    out = np.empty((n_bins, 8))
    _check(load().b9h_mass_function_table(rh.ctypes.data_as(_dp), rh.shape[0], edges.ctypes.data_as(_dp), n_bins, out.ctypes.data_as(_dp)))
    return out


def write_mass_function(path: str, table) -> None:
    """b9h_write_mass_function: the .massFunction file of a per-bin table [n_bins, 8]."""
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, 8)
    _check(load().b9h_write_mass_function(path.encode(), table.ctypes.data_as(_dp), table.shape[0]))


def write_star_mass_hist(path: str, ids, star_hist, n_rows: int) -> None:
    """b9h_write_star_mass_hist: the .starMassHist file of b9_mass_hist's star_hist [len(ids), n_bins + 1] over n_rows rows."""
    sh = np.ascontiguousarray(star_hist, dtype=np.float64).reshape(len(ids), -1)
    arr = (C.c_char_p * len(ids))(*[str(i).encode() for i in ids])
    _check(load().b9h_write_star_mass_hist(path.encode(), arr, len(ids), sh.ctypes.data_as(_dp), sh.shape[1] - 1, int(n_rows)))


def mass_function_settings(args, m_wd_up: float = 8.0):
    """massFunction's settings as the program parses `args` (flags, --config file): (dict of its keys, edges [nBins + 1])."""
    argv = (C.c_char_p * (len(args) + 1))(b"massFunction", *[str(a).encode() for a in args])
    buf = C.create_string_buffer(4096)
    edges = np.zeros(65)
    _check(load().b9h_mass_function_settings(len(args) + 1, argv, float(m_wd_up), buf, 4096, edges.ctypes.data_as(_dp)))
    d = {}
    for line in buf.value.decode().splitlines():
        k, v = line.split(" = ")
        d[k] = float(v) if k in ("minMass", "maxMass") else int(v)
    return d, edges[:d["nBins"] + 1].copy()


BINARY_FRACTION_COLUMNS = ("lo", "hi", "nRows", "N_mean", "N_sd", "N_p16", "N_p50", "N_p84", "f_mean", "f_sd", "f_p16", "f_p50", "f_p84")
RATIO_DIST_COLUMNS = ("j", "q", "nRows", "mean", "sd", "p16", "p50", "p84")


def _row_cells(row_cells, n_mbins: int, Q: int) -> np.ndarray:
    if int(n_mbins) < 1 or int(Q) < 1:
        raise HostError("n_mbins and Q must be positive")
    return np.ascontiguousarray(row_cells, dtype=np.float64).reshape(-1, int(n_mbins) * int(Q) + 1)


def binary_table(row_cells, mass_edges, Q: int, q_min: float = 0.0) -> np.ndarray:
    """b9h_binary_table: b9_ratio_hist's row_cells [n_rows, n_mbins Q + 1] -> [n_mbins + 1, 13] (BINARY_FRACTION_COLUMNS): one
    line per mass bin, then the "all" line; N the line's expected members, f the fraction of them with a companion at
    j >= 1 and j / Q >= q_min."""
    edges = np.ascontiguousarray(mass_edges, dtype=np.float64).reshape(-1)
    n_mbins = len(edges) - 1
    rc = _row_cells(row_cells, n_mbins, Q)
    out = np.empty((n_mbins + 1, 13))
    _check(load().b9h_binary_table(rc.ctypes.data_as(_dp), rc.shape[0], edges.ctypes.data_as(_dp), n_mbins, int(Q), float(q_min), out.ctypes.data_as(_dp)))
    return out


def ratio_dist_table(row_cells, n_mbins: int, Q: int) -> np.ndarray:
    """b9h_ratio_dist_table: row_cells -> [n_mbins + 1, Q, 8] (RATIO_DIST_COLUMNS): per line and ratio node the statistics of
    cell / N over the line's rows."""
    rc = _row_cells(row_cells, n_mbins, Q)
    out = np.empty((int(n_mbins) + 1, int(Q), 8))
    _check(load().b9h_ratio_dist_table(rc.ctypes.data_as(_dp), rc.shape[0], int(n_mbins), int(Q), out.ctypes.data_as(_dp)))
    return out


def star_ratio_table(star_cells, n_mbins: int, Q: int, n_rows_in_grid: int, q_min: float = 0.0) -> np.ndarray:
    """b9h_star_ratio_table: b9_ratio_hist's star_cells [n_stars, n_mbins Q + 1] -> [n_stars, 4 + Q]: rows (= n_rows_in_grid,
    the number of rows the caller summed), member, inRange, pBinaryAbove, then P(q = j / Q | member) for every j."""
    sc = _row_cells(star_cells, n_mbins, Q)
    out = np.empty((sc.shape[0], 4 + int(Q)))
    _check(load().b9h_star_ratio_table(sc.ctypes.data_as(_dp), sc.shape[0], int(n_mbins), int(Q), float(q_min), int(n_rows_in_grid), out.ctypes.data_as(_dp)))
    return out


def write_binary_fraction(path: str, table) -> None:
    """b9h_write_binary_fraction: the .binaryFraction file of a table [n_mbins + 1, 13]."""
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, 13)
    _check(load().b9h_write_binary_fraction(path.encode(), table.ctypes.data_as(_dp), table.shape[0] - 1))


def write_ratio_dist(path: str, table) -> None:
    """b9h_write_ratio_dist: the .ratioDist file of a table [n_mbins + 1, Q, 8]."""
    table = np.ascontiguousarray(table, dtype=np.float64)
    _check(load().b9h_write_ratio_dist(path.encode(), table.ctypes.data_as(_dp), table.shape[0] - 1, table.shape[1]))


def write_star_ratio(path: str, ids, table) -> None:
    """b9h_write_star_ratio: the .starRatio file of a table [len(ids), 4 + Q]."""
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(len(ids), -1)
    arr = (C.c_char_p * len(ids))(*[str(i).encode() for i in ids])
    _check(load().b9h_write_star_ratio(path.encode(), arr, len(ids), table.ctypes.data_as(_dp), table.shape[1] - 4))


STAR_INTERVALS_LEVELS = (0.025, 0.16, 0.5, 0.84, 0.975)
SIV_NO_MASS, SIV_OPEN = 1, 2


def refine_star_edges(edges, acc, levels=STAR_INTERVALS_LEVELS, tol: float = 1e-4) -> dict:
    """b9h_refine_star_edges: one pass of the per-star refinement, a pure function of that pass's edges [n, B + 1], b9_star_bins'
    acc [n, B + 3] and the levels.  Returns lo, hi, below, inside, value, final [n, m], flags [n] (SIV_*) and next_edges [n, B + 1]."""
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    n, ne = edges.shape
    acc = np.ascontiguousarray(acc, dtype=np.float64).reshape(n, ne + 2)
    lv = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    m = len(lv)
    out = {k: np.zeros((n, m)) for k in ("lo", "hi", "below", "inside", "value")}
    fin, flags, nxt = np.zeros((n, m), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, ne))
    _check(load().b9h_refine_star_edges(edges.ctypes.data_as(_dp), acc.ctypes.data_as(_dp), n, ne - 1, lv.ctypes.data_as(_dp), m, float(tol),
                                        *[out[k].ctypes.data_as(_dp) for k in ("lo", "hi", "below", "inside", "value")],
                                        fin.ctypes.data_as(_ip), flags.ctypes.data_as(_ip), nxt.ctypes.data_as(_dp)))
    out.update(final=fin, flags=flags, next_edges=nxt)
    return out


def interval_loop(bins, first_lo, first_hi, n_rows: int, levels=STAR_INTERVALS_LEVELS, tol: float = 1e-4, max_passes: int = 12,
                  n_bins: int = abi.SBIN_MAX_BINS) -> dict:
    """The refinement loop over n independent lines: the first pass cuts [first_lo[i], first_hi[i]] evenly into n_bins bins,
    `bins(edges [n, B + 1]) -> acc [n, B + 3]` bins all the rows from zeros, refine_star_edges narrows every line's edges, until
    every bracket is final or max_passes is reached.  Returns levels, member [n] (the total over n_rows), counted [n] (the
    counted mass over the total, 0 without a total), value, lo, hi, final [n, m], passes [n] (the pass at which the line was
    finished), flags [n] (SIV_*), n_passes, edges (the last), acc (the last)."""
    lo, hi = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (first_lo, first_hi))
    n, B = len(lo), int(n_bins)
    if max_passes < 1:
        raise ValueError("max_passes must be positive")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError("the first ranges must be finite and not empty")
    edges = lo[:, None] + (hi - lo)[:, None] * (np.arange(B + 1, dtype=np.float64) / float(B))[None, :]
    passes = np.zeros(n, dtype=np.int32)
    for k in range(1, int(max_passes) + 1):
        acc = np.ascontiguousarray(bins(edges), dtype=np.float64).reshape(n, B + 3)
        r = refine_star_edges(edges, acc, levels, tol)
        done = (r["flags"] & SIV_OPEN) == 0
        passes[(passes == 0) & (done | (k == max_passes))] = k
        if done.all():
            break
        if k < max_passes:
            edges = r["next_edges"]
    member = acc[:, B + 2] / n_rows if n_rows else np.zeros(n)
    c = np.zeros(n)
    for b in range(B + 2):                      # (refine_star_edges' order: below, the bins, at or above)
        c = c + acc[:, b]
    counted = np.divide(c, acc[:, B + 2], out=np.zeros(n), where=acc[:, B + 2] > 0.0)
    return dict(levels=np.array(levels, dtype=np.float64), member=member, counted=counted, value=r["value"], lo=r["lo"], hi=r["hi"], final=r["final"],
                passes=passes, flags=r["flags"], n_passes=k, edges=edges, acc=acc)


def star_intervals(engine, rows, quantity: int = abi.HQ_PRIMARY, levels=STAR_INTERVALS_LEVELS, tol: float = 1e-4, max_passes: int = 12,
                   n_bins: int = abi.SBIN_MAX_BINS) -> dict:
    """Every star's quantiles of `quantity` at `levels` over `rows`, exactly: loops engine.star_bins (b9_star_bins; anything
    with star_bins(rows, edges, quantity), n_stars and max_mass serves) and refine_star_edges until every bracket is final or
    max_passes is reached (interval_loop).  The first pass's edges are [0, 2 engine.max_mass] cut evenly for every star.  Returns
    levels, member [n], value, lo, hi, final [n, m], passes [n] (the pass at which the star was finished), flags [n] (SIV_*),
    n_passes, edges (the last)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    n = int(engine.n_stars)
    return interval_loop(lambda edges: engine.star_bins(rows, edges, quantity), np.zeros(n), np.full(n, 2.0 * float(engine.max_mass)),
                         rows.shape[0], levels, tol, max_passes, n_bins)


def star_intervals_table(res: dict) -> np.ndarray:
    """b9h_star_intervals_table: star_intervals' result -> [n, 3 m + 3]: member, then value, lo, hi per level, passes, flags."""
    n, m = res["value"].shape
    c = lambda a, t: np.ascontiguousarray(a, dtype=t)      # noqa: E731
    member, value, lo, hi = (c(res[k], np.float64) for k in ("member", "value", "lo", "hi"))
    passes, flags = c(res["passes"], np.int32), c(res["flags"], np.int32)
    out = np.zeros((n, 3 * m + 3))
    _check(load().b9h_star_intervals_table(n, m, member.ctypes.data_as(_dp), value.ctypes.data_as(_dp), lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp),
                                           passes.ctypes.data_as(_ip), flags.ctypes.data_as(_ip), out.ctypes.data_as(_dp)))
    return out


def write_star_intervals(path: str, ids, levels, table) -> None:
    """b9h_write_star_intervals: the .starIntervals file of star_intervals_table's table [len(ids), 3 m + 3]."""
    lv = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(len(ids), 3 * len(lv) + 3)
    arr = (C.c_char_p * len(ids))(*[str(i).encode() for i in ids])
    _check(load().b9h_write_star_intervals(path.encode(), arr, len(ids), lv.ctypes.data_as(_dp), len(lv), table.ctypes.data_as(_dp)))


def read_star_intervals(path: str):
    """(ids, columns, table [n, 3 m + 3]) of a .starIntervals file."""
    return read_table_file(path, "id")


def star_intervals_settings(args) -> dict:
    """starIntervals' settings as the program parses `args` (flags, --config file): a dict of its keys (levels: a tuple)."""
    argv = (C.c_char_p * (len(args) + 1))(b"starIntervals", *[str(a).encode() for a in args])
    buf = C.create_string_buffer(4096)
    _check(load().b9h_star_intervals_settings(len(args) + 1, argv, buf, 4096))
    d = {}
    for line in buf.value.decode().splitlines():
        k, v = line.split(" = ")
        d[k] = tuple(float(x) for x in v.split(",")) if k == "levels" else float(v) if k == "tol" else int(v)
    return d


WD_QUANTITY_NAMES = ("zamsMass", "wdMass", "precLogAge", "logCoolAge", "logTeff", "logg")


def wd_quantity_mask(quantities) -> int:
    """The mask of b9_wd_bins for an int (taken as it is) or for names of WD_QUANTITY_NAMES."""
    if isinstance(quantities, (int, np.integer)):
        return int(quantities)
    mask = 0
    for q in quantities:
        mask |= 1 << WD_QUANTITY_NAMES.index(q)
    return mask


def wd_first_ranges(wd_acc, quantities=abi.WQ_ALL):
    """b9h_wd_first_ranges: the lines' first ranges (lo, hi) [n_wd, n_sel] from b9_wd_moments' accumulators [n_wd, 16]: the
    quantity's mean over its counted mass -/+ max(6 sd, 1e-3 |mean|); [0, 1] without counted mass."""
    mask = wd_quantity_mask(quantities)
    acc = np.ascontiguousarray(wd_acc, dtype=np.float64).reshape(-1, abi.WDM_N)
    n_sel = bin(mask).count("1")
    lo, hi = np.zeros((acc.shape[0], n_sel)), np.zeros((acc.shape[0], n_sel))
    _check(load().b9h_wd_first_ranges(acc.ctypes.data_as(_dp), acc.shape[0], mask, lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp)))
    return lo, hi


def wd_intervals(engine, rows, n_nodes: int = 512, quantities=abi.WQ_ALL, levels=STAR_INTERVALS_LEVELS, tol: float = 1e-4,
                 max_passes: int = 12) -> dict:
    """Every WD-stage star's quantiles of the selected quantities at `levels` over `rows` on the grid of n_nodes steps, exactly:
    one engine.wd_moments pass gives every line (star, quantity) its first range (wd_first_ranges), then engine.wd_bins
    (b9_wd_bins) and refine_star_edges are looped (interval_loop) until every bracket is final or max_passes is reached --
    the program wdIntervals' loop.  Returns interval_loop's dict over the n_wd * n_sel lines (member, counted, passes, flags
    [n_wd * n_sel]; value, lo, hi, final [n_wd * n_sel, m]) with n_wd, n_sel, quantities (the mask), star_index, first_lo, first_hi."""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    mask = wd_quantity_mask(quantities)
    n_sel = bin(mask).count("1")
    wd_acc, star_index = engine.wd_moments(rows, n_nodes)
    n_wd = wd_acc.shape[0]
    lo, hi = wd_first_ranges(wd_acc, mask)
    res = interval_loop(lambda edges: engine.wd_bins(rows, n_nodes, edges.reshape(n_wd, n_sel, -1), mask)[0], lo.reshape(-1), hi.reshape(-1),
                        rows.shape[0], levels, tol, max_passes, abi.WBIN_MAX_BINS)
    res.update(n_wd=n_wd, n_sel=n_sel, quantities=mask, star_index=star_index, first_lo=lo, first_hi=hi)
    return res


def wd_intervals_table(res: dict) -> np.ndarray:
    """b9h_wd_intervals_table: wd_intervals' result -> [n_wd, 1 + n_sel (3 m + 3)]: member, then per selected quantity counted,
    {value, lo, hi} per level, passes, flags."""
    n_wd, n_sel = int(res["n_wd"]), int(res["n_sel"])
    m = res["value"].shape[1]
    c = lambda a, t: np.ascontiguousarray(a, dtype=t)      # noqa: E731
    member, counted, value, lo, hi = (c(res[k], np.float64) for k in ("member", "counted", "value", "lo", "hi"))
    passes, flags = c(res["passes"], np.int32), c(res["flags"], np.int32)
    out = np.zeros((n_wd, 1 + n_sel * (3 * m + 3)))
    _check(load().b9h_wd_intervals_table(n_wd, n_sel, m, member.ctypes.data_as(_dp), counted.ctypes.data_as(_dp), value.ctypes.data_as(_dp),
                                         lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp), passes.ctypes.data_as(_ip), flags.ctypes.data_as(_ip),
                                         out.ctypes.data_as(_dp)))
    return out


def write_wd_intervals(path: str, ids, quantities, levels, table) -> None:
    """b9h_write_wd_intervals: the .wdIntervals file of wd_intervals_table's table [len(ids), 1 + n_sel (3 m + 3)]."""
    mask = wd_quantity_mask(quantities)
    lv = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(len(ids), 1 + bin(mask).count("1") * (3 * len(lv) + 3))
    arr = (C.c_char_p * len(ids))(*[str(i).encode() for i in ids])
    _check(load().b9h_write_wd_intervals(path.encode(), arr, len(ids), mask, lv.ctypes.data_as(_dp), len(lv), table.ctypes.data_as(_dp)))


def read_wd_intervals(path: str):
    """(ids, columns, table [n_wd, 1 + n_sel (3 m + 3)]) of a .wdIntervals file."""
    return read_table_file(path, "id")


def wd_intervals_settings(args) -> dict:
    """wdIntervals' settings as the program parses `args` (flags, --config file): a dict of its keys (quantities: the mask;
    levels: a tuple)."""
    argv = (C.c_char_p * (len(args) + 1))(b"wdIntervals", *[str(a).encode() for a in args])
    buf = C.create_string_buffer(4096)
    _check(load().b9h_wd_intervals_settings(len(args) + 1, argv, buf, 4096))
    d = {}
    for line in buf.value.decode().splitlines():
        k, v = line.split(" = ")
        d[k] = tuple(float(x) for x in v.split(",")) if k == "levels" else float(v) if k == "tol" else int(v)
    return d


def band_first_ranges(mom):
    """b9h_band_first_ranges: every line's first range (lo, hi) [n_lines] from b9_cmd_band's moments [n_lines, 5]: [MIN - pad,
    MAX + pad] with pad = max(0.01 (MAX - MIN), 1e-6 max(1, |MIN|, |MAX|)); [0, 1] for a line with N = 0.  What interval_loop cuts."""
    mom = np.ascontiguousarray(mom, dtype=np.float64).reshape(-1, abi.BAND_NMOM)
    lo, hi = np.zeros(mom.shape[0]), np.zeros(mom.shape[0])
    _check(load().b9h_band_first_ranges(mom.ctypes.data_as(_dp), mom.shape[0], lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp)))
    return lo, hi


def band_first_edges(mom, n_bins: int = abi.BAND_MAX_BINS) -> np.ndarray:
    """b9h_band_first_edges: every line's first edges [n_lines, n_bins + 1] from b9_cmd_band's moments [n_lines, 5]: strictly
    ascending, e_0 < MIN and e_B > MAX; [0, 1] cut evenly for a line with N = 0."""
    mom = np.ascontiguousarray(mom, dtype=np.float64).reshape(-1, abi.BAND_NMOM)
    edges = np.zeros((mom.shape[0], int(n_bins) + 1))
    _check(load().b9h_band_first_edges(mom.ctypes.data_as(_dp), mom.shape[0], int(n_bins), edges.ctypes.data_as(_dp)))
    return edges


def cmd_band(engine, rows, spec, levels=STAR_INTERVALS_LEVELS, tol: float = 1e-4, max_passes: int = 12, n_bins: int = abi.BAND_MAX_BINS) -> dict:
    """Every line's moments and quantiles at `levels` over `rows`, exactly -- the program cmdBand's loop: engine.cmd_band
    (b9_cmd_band) on the first row gives the pivots (that row's value, 0 where the line is absent there), one pass over all the
    rows the moments about them, band_first_ranges the first ranges (interval_loop's even cut of them is band_first_edges), then the
    bins pass and refine_star_edges are looped (interval_loop) until every bracket is final or max_passes is reached.  Returns
    interval_loop's dict over the lines with pivot [n_lines], mom [n_lines, 5], first_lo and first_hi [n_lines]."""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    first, _ = engine.cmd_band(rows[:1], spec)
    pivot = np.where(first[:, abi.BAND_N] > 0.0, first[:, abi.BAND_MIN], 0.0)
    mom, _ = engine.cmd_band(rows, spec, pivot=pivot)
    lo, hi = band_first_ranges(mom)
    res = interval_loop(lambda e: engine.cmd_band(rows, spec, edges=e, want_mom=False)[1], lo, hi, rows.shape[0], levels, tol, max_passes, n_bins)
    res.update(pivot=pivot, mom=mom, first_lo=lo, first_hi=hi)
    return res


def band_table(res: dict) -> np.ndarray:
    """b9h_band_table: cmd_band's result -> [n_lines, 5 + 3 m + 2]: N, mean, sd, min, max, then value, lo, hi per level, passes,
    flags."""
    n, m = res["value"].shape
    c = lambda a, t: np.ascontiguousarray(a, dtype=t)      # noqa: E731
    mom, pivot, value, lo, hi = (c(res[k], np.float64) for k in ("mom", "pivot", "value", "lo", "hi"))
    passes, flags = c(res["passes"], np.int32), c(res["flags"], np.int32)
    out = np.zeros((n, 5 + 3 * m + 2))
    _check(load().b9h_band_table(mom.ctypes.data_as(_dp), pivot.ctypes.data_as(_dp), n, m, value.ctypes.data_as(_dp), lo.ctypes.data_as(_dp),
                                 hi.ctypes.data_as(_dp), passes.ctypes.data_as(_ip), flags.ctypes.data_as(_ip), out.ctypes.data_as(_dp)))
    return out


def write_cmd_band(path: str, names, levels, table) -> None:
    """b9h_write_cmd_band: the .cmdBand file of band_table's table [len(names), 5 + 3 m + 2]."""
    lv = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(len(names), 5 + 3 * len(lv) + 2)
    arr = (C.c_char_p * len(names))(*[str(i).encode() for i in names])
    _check(load().b9h_write_cmd_band(path.encode(), arr, len(names), lv.ctypes.data_as(_dp), len(lv), table.ctypes.data_as(_dp)))


def read_cmd_band(path: str):
    """(line names, columns, table [n_lines, 5 + 3 m + 2]) of a .cmdBand file."""
    return read_table_file(path, "line")


def cmd_band_settings(args) -> dict:
    """cmdBand's settings as the program parses `args` (flags, --config file): a dict of its keys (ratios, levels: tuples of
    floats; colours: a tuple of "f1-f2" strings; wdTypes: the mask)."""
    argv = (C.c_char_p * (len(args) + 1))(b"cmdBand", *[str(a).encode() for a in args])
    buf = C.create_string_buffer(4096)
    _check(load().b9h_cmd_band_settings(len(args) + 1, argv, buf, 4096))
    d = {}
    for line in buf.value.decode().splitlines():
        k, _, v = line.partition(" = ")
        v = v.strip()
        if k in ("ratios", "levels"):
            d[k] = tuple(float(x) for x in v.split(",")) if v else ()
        elif k == "colours":
            d[k] = tuple(v.split(",")) if v else ()
        else:
            d[k] = float(v) if k == "tol" else int(v)
    return d


def read_table_file(path: str, first: str):
    """(labels of the first column, columns, values [lines, len(columns)]) of a whitespace table with one header line;
    first: the header's first word ("id" for .starMassHist; None: every column is a number, as in .massFunction)."""
    with open(path) as f:
        header = f.readline().split()
        skip = 0 if first is None else 1
        if first is not None and header[:1] != [first]:
            raise HostError(path + ": unexpected header")
        labels, rows = [], []
        for line in f:
            t = line.split()
            if not t:
                continue
            if len(t) != len(header):
                raise HostError(path + ": a line does not hold one value per column")
            labels.append(t[0])
            rows.append([float(x) for x in t[skip:]])
    return labels, header[skip:], np.array(rows, dtype=np.float64).reshape(len(rows), len(header) - skip)


RESID_STAR_COLUMNS = ("predMag", "predSd", "resid", "rmsZ")
FILTER_RESID_COLUMNS = ("nRows",) + tuple(q + "_" + s for q in ("meanZ", "chi2", "offset") for s in ("mean", "sd", "p16", "p50", "p84"))


def resid_table(star_resid, obs, sigma) -> np.ndarray:
    """b9h_resid_table: b9_phot_resid's star_resid [n_stars, 2 + 2 nf] with the catalogue's obs / sigma [n_stars, nf] -> the
    per-star table [n_stars, 2 + 4 nf]: rows, member, then RESID_STAR_COLUMNS per filter."""
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    n, nf = obs.shape
    sigma = np.ascontiguousarray(sigma, dtype=np.float64).reshape(n, nf)
    sr = np.ascontiguousarray(star_resid, dtype=np.float64).reshape(n, 2 + 2 * nf)
    out = np.empty((n, 2 + 4 * nf))
    _check(load().b9h_resid_table(sr.ctypes.data_as(_dp), obs.ctypes.data_as(_dp), sigma.ctypes.data_as(_dp), n, nf, out.ctypes.data_as(_dp)))
    return out


def filter_resid_table(row_resid, n_filt: int) -> np.ndarray:
    """b9h_filter_resid_table: b9_phot_resid's row_resid [n_rows, 1 + 5 nf] -> the per-filter table [nf, 16] (FILTER_RESID_COLUMNS)."""
    rr = np.ascontiguousarray(row_resid, dtype=np.float64).reshape(-1, 1 + 5 * n_filt)
    out = np.empty((n_filt, 16))
    _check(load().b9h_filter_resid_table(rr.ctypes.data_as(_dp), rr.shape[0], int(n_filt), out.ctypes.data_as(_dp)))
    return out


def _names(v):
    return (C.c_char_p * len(v))(*[str(i).encode() for i in v])


def write_phot_resid(path: str, ids, filters, table) -> None:
    """b9h_write_phot_resid: the .photResid file of a per-star table [len(ids), 2 + 4 len(filters)]."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(len(ids), 2 + 4 * len(filters))
    _check(load().b9h_write_phot_resid(path.encode(), _names(ids), len(ids), _names(filters), len(filters), t.ctypes.data_as(_dp)))


def write_filter_resid(path: str, filters, table) -> None:
    """b9h_write_filter_resid: the .filterResid file of a per-filter table [len(filters), 16]."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(len(filters), 16)
    _check(load().b9h_write_filter_resid(path.encode(), _names(filters), len(filters), t.ctypes.data_as(_dp)))


def read_phot_resid(path: str):
    """(ids, columns, table [n_stars, 2 + 4 nf]) of a .photResid file."""
    return read_table_file(path, "id")


def read_filter_resid(path: str):
    """(filters, columns, table [nf, 16]) of a .filterResid file."""
    return read_table_file(path, "filter")


def phot_resid_settings(args):
    """photResiduals' settings as the program parses `args` (flags, --config file): a dict of its four keys."""
    argv = (C.c_char_p * (len(args) + 1))(b"photResiduals", *[str(a).encode() for a in args])
    buf = C.create_string_buffer(1024)
    _check(load().b9h_phot_resid_settings(len(args) + 1, argv, buf, 1024))
    return {k: int(v) for k, v in (line.split(" = ") for line in buf.value.decode().splitlines())}


LOO_STAR_COLUMNS = ("looMag", "looSd", "resid", "z", "lpd")
FILTER_CHECK_COLUMNS = ("nRows",) + tuple(q + "_" + s for q in ("meanZ", "chi2", "offset", "lpd") for s in ("mean", "sd", "p16", "p50", "p84"))


def loo_table(star_loo, obs, sigma) -> np.ndarray:
    """b9h_loo_table: b9_filter_loo's star_loo [n_stars, 2 + 3 nf] with the catalogue's obs / sigma [n_stars, nf] -> the
    per-star table [n_stars, 2 + 5 nf]: rows, member, then LOO_STAR_COLUMNS per filter."""
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    n, nf = obs.shape
    sigma = np.ascontiguousarray(sigma, dtype=np.float64).reshape(n, nf)
    sl = np.ascontiguousarray(star_loo, dtype=np.float64).reshape(n, 2 + 3 * nf)
    out = np.empty((n, 2 + 5 * nf))
    _check(load().b9h_loo_table(sl.ctypes.data_as(_dp), obs.ctypes.data_as(_dp), sigma.ctypes.data_as(_dp), n, nf, out.ctypes.data_as(_dp)))
    return out


def filter_loo_table(row_loo, n_filt: int) -> np.ndarray:
    """b9h_filter_loo_table: b9_filter_loo's row_loo [n_rows, 1 + 6 nf] -> the per-filter table [nf, 21] (FILTER_CHECK_COLUMNS)."""
    rl = np.ascontiguousarray(row_loo, dtype=np.float64).reshape(-1, 1 + 6 * n_filt)
    out = np.empty((n_filt, 21))
    _check(load().b9h_filter_loo_table(rl.ctypes.data_as(_dp), rl.shape[0], int(n_filt), out.ctypes.data_as(_dp)))
    return out


def write_star_filter_check(path: str, ids, filters, table) -> None:
    """b9h_write_star_filter_check: the .starFilterCheck file of a per-star table [len(ids), 2 + 5 len(filters)]."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(len(ids), 2 + 5 * len(filters))
    _check(load().b9h_write_star_filter_check(path.encode(), _names(ids), len(ids), _names(filters), len(filters), t.ctypes.data_as(_dp)))


def write_filter_check(path: str, filters, table) -> None:
    """b9h_write_filter_check: the .filterCheck file of a per-filter table [len(filters), 21]."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(len(filters), 21)
    _check(load().b9h_write_filter_check(path.encode(), _names(filters), len(filters), t.ctypes.data_as(_dp)))


def read_star_filter_check(path: str):
    """(ids, columns, table [n_stars, 2 + 5 nf]) of a .starFilterCheck file."""
    return read_table_file(path, "id")


def read_filter_check(path: str):
    """(filters, columns, table [nf, 21]) of a .filterCheck file."""
    return read_table_file(path, "filter")


def filter_check_settings(args):
    """filterCheck's settings as the program parses `args` (flags, --config file): a dict of its four keys."""
    argv = (C.c_char_p * (len(args) + 1))(b"filterCheck", *[str(a).encode() for a in args])
    buf = C.create_string_buffer(1024)
    _check(load().b9h_filter_check_settings(len(args) + 1, argv, buf, 1024))
    return {k: int(v) for k, v in (line.split(" = ") for line in buf.value.decode().splitlines())}


OFFSET_STAR_COLUMNS = ("mean", "sd", "z", "logBF")
OFFSET_DIST_COLUMNS = ("nRows",) + tuple(q + "_" + s for q in ("mean", "rms", "logBF") for s in ("mean", "sd", "p16", "p50", "p84"))


def offset_direction(spec, filters, abs_coeff=None) -> np.ndarray:
    """b9h_offset_direction: k [len(filters)] of a direction: "absorption" (k = abs_coeff: more dust at the same true
    distance), "distance" (k = 1), "filter:NAME" (a unit vector), or an explicit list of values (a sequence, or a
    comma-separated string)."""
    if not isinstance(spec, str):
        spec = ",".join(repr(float(v)) for v in spec)
    nf = len(filters)
    ac = None if abs_coeff is None else np.ascontiguousarray(abs_coeff, dtype=np.float64).reshape(nf)
    out = np.empty(nf)
    _check(load().b9h_offset_direction(spec.encode(), _names(filters), nf, None if ac is None else ac.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
    return out


def offset_directions(specs, filters, abs_coeff=None) -> np.ndarray:
    """k [len(specs), len(filters)] of several directions (offset_direction each): what Engine.star_offset takes."""
    return np.stack([offset_direction(s, filters, abs_coeff) for s in specs])


def offset_table(star_off, sigma, k, tau) -> np.ndarray:
    """b9h_offset_table: b9_star_offset's star_off [n_stars, 2 + 3 D] with the catalogue's sigma [n_stars, nf] and the call's
    k [D, nf], tau [D] (a scalar serves every direction) -> the per-star table [n_stars, 2 + 4 D]: rows, member, then
    OFFSET_STAR_COLUMNS per direction."""
    sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    n, nf = sigma.shape
    k = np.ascontiguousarray(k, dtype=np.float64).reshape(-1, nf)
    nd = k.shape[0]
    tau = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, dtype=np.float64), (nd,)))
    so = np.ascontiguousarray(star_off, dtype=np.float64).reshape(n, 2 + 3 * nd)
    out = np.empty((n, 2 + 4 * nd))
    _check(load().b9h_offset_table(so.ctypes.data_as(_dp), sigma.ctypes.data_as(_dp), k.ctypes.data_as(_dp), tau.ctypes.data_as(_dp), n, nf, nd,
                                   out.ctypes.data_as(_dp)))
    return out


def offset_dist_table(row_off, n_dir: int) -> np.ndarray:
    """b9h_offset_dist_table: b9_star_offset's row_off [n_rows, 1 + 4 D] -> the per-direction table [D, 16] (OFFSET_DIST_COLUMNS)."""
    ro = np.ascontiguousarray(row_off, dtype=np.float64).reshape(-1, 1 + 4 * n_dir)
    out = np.empty((n_dir, 16))
    _check(load().b9h_offset_dist_table(ro.ctypes.data_as(_dp), ro.shape[0], int(n_dir), out.ctypes.data_as(_dp)))
    return out


def write_star_offsets(path: str, ids, directions, table) -> None:
    """b9h_write_star_offsets: the .starOffsets file of a per-star table [len(ids), 2 + 4 len(directions)]."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(len(ids), 2 + 4 * len(directions))
    _check(load().b9h_write_star_offsets(path.encode(), _names(ids), len(ids), _names(directions), len(directions), t.ctypes.data_as(_dp)))


def write_offset_dist(path: str, directions, table) -> None:
    """b9h_write_offset_dist: the .offsetDist file of a per-direction table [len(directions), 16]."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(len(directions), 16)
    _check(load().b9h_write_offset_dist(path.encode(), _names(directions), len(directions), t.ctypes.data_as(_dp)))


def read_star_offsets(path: str):
    """(ids, columns, table [n_stars, 2 + 4 D]) of a .starOffsets file."""
    return read_table_file(path, "id")


def read_offset_dist(path: str):
    """(directions, columns, table [D, 16]) of an .offsetDist file."""
    return read_table_file(path, "direction")


def star_offsets_settings(args):
    """starOffsets' settings as the program parses `args` (flags, --config file): margIsoIncrem, nMassRatios, nPops (ints),
    direction (a list of specs) and tau (a list of floats, one per direction)."""
    argv = (C.c_char_p * (len(args) + 1))(b"starOffsets", *[str(a).encode() for a in args])
    buf = C.create_string_buffer(2048)
    _check(load().b9h_star_offsets_settings(len(args) + 1, argv, buf, 2048))
    d = dict(line.split(" = ") for line in buf.value.decode().splitlines())
    return dict(margIsoIncrem=int(d["margIsoIncrem"]), nMassRatios=int(d["nMassRatios"]), nPops=int(d["nPops"]),
                direction=d["direction"].split(), tau=[float(v) for v in d["tau"].split()])


POINTWISE_COLUMNS = ("rows", "nInf", "lppd", "pWaic", "elpdWaic", "elpdIs", "paretoK", "elpdLoo", "pLoo")
SCORE_TOTALS = ("nStars", "lppd", "lppdSe", "elpdWaic", "elpdWaicSe", "elpdLoo", "elpdLooSe", "pWaic", "pLoo", "nInfStars", "nHighK", "maxK")
SCORE_COMPARE = ("nStars", "dElpdLoo", "dElpdLooSe", "dElpdWaic", "dElpdWaicSe", "nDropped")


def pointwise_table(acc, tail=None) -> np.ndarray:
    """b9h_pointwise_table: b9_pointwise's acc [n_stars, 8] and tail [n_stars, tail_len] (None: no PSIS fit) -> the per-star
    table [n_stars, 9] (POINTWISE_COLUMNS)."""
    a = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1, 8)
    n = a.shape[0]
    t = None if tail is None else np.ascontiguousarray(tail, dtype=np.float64).reshape(n, -1)
    out = np.empty((n, len(POINTWISE_COLUMNS)))
    _check(load().b9h_pointwise_table(a.ctypes.data_as(_dp), t.ctypes.data_as(_dp) if t is not None else None, 0 if t is None else t.shape[1], n,
                                      out.ctypes.data_as(_dp)))
    return out


def score_totals(table) -> dict:
    """b9h_score_totals: the totals of a per-star table over its stars with rows > 0 (SCORE_TOTALS)."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, len(POINTWISE_COLUMNS))
    out = np.empty(len(SCORE_TOTALS))
    _check(load().b9h_score_totals(t.ctypes.data_as(_dp), t.shape[0], out.ctypes.data_as(_dp)))
    return dict(zip(SCORE_TOTALS, out.tolist()))


def score_compare(table_a, ids_a, table_b, ids_b) -> dict:
    """b9h_score_compare: the paired difference A - B of two per-star tables of the same catalogue (SCORE_COMPARE); HostError
    when the star ids differ in content or order."""
    a = np.ascontiguousarray(table_a, dtype=np.float64).reshape(len(ids_a), len(POINTWISE_COLUMNS))
    b = np.ascontiguousarray(table_b, dtype=np.float64).reshape(len(ids_b), len(POINTWISE_COLUMNS))
    out = np.empty(len(SCORE_COMPARE))
    _check(load().b9h_score_compare(a.ctypes.data_as(_dp), _names(ids_a), len(ids_a), b.ctypes.data_as(_dp), _names(ids_b), len(ids_b),
                                    out.ctypes.data_as(_dp)))
    return dict(zip(SCORE_COMPARE, out.tolist()))


def write_pointwise(path: str, ids, table) -> None:
    """b9h_write_pointwise: the .pointwise file of a per-star table [len(ids), 9]."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(len(ids), len(POINTWISE_COLUMNS))
    _check(load().b9h_write_pointwise(path.encode(), _names(ids), len(ids), t.ctypes.data_as(_dp)))


def write_model_score(path: str, totals) -> None:
    """b9h_write_model_score: the .modelScore file of score_totals' values."""
    v = np.array([totals[k] for k in SCORE_TOTALS] if isinstance(totals, dict) else totals, dtype=np.float64)
    _check(load().b9h_write_model_score(path.encode(), v.ctypes.data_as(_dp)))


def read_pointwise(path: str):
    """(ids, columns, table [n_stars, 9]) of a .pointwise file."""
    return read_table_file(path, "id")


def read_named_values(path: str) -> dict:
    """A .modelScore / .modelCompare file (one header line, one line of values) as a dict."""
    with open(path) as f:
        names, values = f.readline().split(), f.readline().split()
    return dict(zip(names, (float(v) for v in values)))


def read_row_lpd(path: str) -> np.ndarray:
    """The lpd column of a .rowLpd file."""
    with open(path) as f:
        assert f.readline().split() == ["row", "lpd"]
        return np.array([float(line.split()[1]) for line in f if line.strip()])


def model_score_settings(args):
    """modelScore's settings as the program parses `args` (flags, --config file): a dict of its five keys."""
    argv = (C.c_char_p * (len(args) + 1))(b"modelScore", *[str(a).encode() for a in args])
    buf = C.create_string_buffer(4096)
    _check(load().b9h_model_score_settings(len(args) + 1, argv, buf, 4096))
    d = dict(line.split(" = ") if " = " in line else (line.rstrip(" ="), "") for line in buf.value.decode().splitlines())
    return {k: (v if k == "compareTo" else int(v)) for k, v in d.items()}


# ------------------------------------------------------------------------------------------
# simCluster / scatterCluster draws (b9sim.hpp; docs/FORMATS.md "Simulation draws")
# ------------------------------------------------------------------------------------------
def sim_draw_systems(seed: int, i0: int, n: int, tip, min_mass: float = 0.1, max_mass: float = 8.0, percent_binary: float = 0.0,
                     min_mass_ratio: float = 0.0, percent_db: float = 0.0, n_pops: int = 1, lam: float = 0.5):
    """Systems i0 .. i0+n-1 of simCluster: (mass1, mass_ratio, wd_type, pop).  tip: AGB-tip mass per population."""
    t = np.atleast_1d(np.asarray(tip, dtype=np.float64))
    tips = np.array([t[0], t[-1]])
    m1, q = np.empty(n), np.empty(n)
    wt, pop = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    _check(load().b9h_sim_draw_systems(int(seed), int(i0), int(n), float(min_mass), float(max_mass), float(percent_binary),
                                       float(min_mass_ratio), float(percent_db), int(n_pops), float(lam), tips.ctypes.data_as(_dp),
                                       m1.ctypes.data_as(_dp), q.ctypes.data_as(_dp), wt.ctypes.data_as(_ip), pop.ctypes.data_as(_ip)))
    return m1, q, wt, pop


def sim_field_mags(seed: int, i0: int, n: int, lo, hi) -> np.ndarray:
    """Field-star magnitudes [n, n_filt] of systems i0 .. i0+n-1: uniform in [lo, hi] per filter."""
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    out = np.empty((n, lo.size))
    _check(load().b9h_sim_field_mags(int(seed), int(i0), int(n), lo.size, lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp),
                                     out.ctypes.data_as(_dp)))
    return out


def scatter(seed: int, ids, mags, sigma_floor: float, sigma_at_limit: float, faint_limit: float):
    """scatterCluster's noise: (sigma, obs), each [n, n_filt], for systems `ids` with noiseless magnitudes `mags`."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    mags = np.ascontiguousarray(mags, dtype=np.float64).reshape(ids.size, -1)
    sigma, obs = np.empty_like(mags), np.empty_like(mags)
    _check(load().b9h_scatter(int(seed), ids.ctypes.data_as(C.POINTER(C.c_int64)), ids.size, mags.shape[1], mags.ctypes.data_as(_dp),
                              float(sigma_floor), float(sigma_at_limit), float(faint_limit), sigma.ctypes.data_as(_dp), obs.ctypes.data_as(_dp)))
    return sigma, obs


def sim_settings(program: str, args: Sequence[str]) -> dict:
    """The resolved, checked settings of a simCluster / scatterCluster command line (args without the program name)."""
    argv = [program.encode()] + [a.encode() for a in args]
    arr = (C.c_char_p * len(argv))(*argv)
    buf = C.create_string_buffer(8192)
    _check(load().b9h_sim_settings(0 if program == "simCluster" else 1, len(argv), arr, buf, len(buf)))
    out = {}
    for line in buf.value.decode().splitlines():
        k, v = line.split(" = ", 1)
        out[k] = float(v)
    return out


INFLUENCE_HEAD = ("rows", "nInf", "ess", "paretoK")
GROUP_INFLUENCE_HEAD = ("nStars", "rows", "nInf", "ess", "paretoK")


def influence_table(acc, tail=None) -> np.ndarray:
    """b9h_influence_table: b9_star_influence's acc [n_stars, 6 + 4 Q] and tail [n_stars, tail_len] (None: no PSIS fit) -> the
    per-star table [n_stars, 4 + 3 Q]: INFLUENCE_HEAD, then shift, lin, looSd per quantity."""
    a = np.ascontiguousarray(acc, dtype=np.float64)
    n, nq = a.shape[0], (a.shape[1] - 6) // 4
    t = None if tail is None else np.ascontiguousarray(tail, dtype=np.float64).reshape(n, -1)
    out = np.empty((n, 4 + 3 * nq))
    _check(load().b9h_influence_table(a.ctypes.data_as(_dp), t.ctypes.data_as(_dp) if t is not None else None, 0 if t is None else t.shape[1], n, nq,
                                      out.ctypes.data_as(_dp)))
    return out


def group_influence_table(group_lpd, q, groups) -> np.ndarray:
    """b9h_group_influence_table: b9_star_influence's group_lpd [n_rows, G], the call's q [n_rows, Q] and the stars' group ids ->
    the per-group table [G, 5 + 3 Q]: GROUP_INFLUENCE_HEAD, then shiftRaw, shift, looSd per quantity."""
    L = np.ascontiguousarray(group_lpd, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(L.shape[0], -1)
    g = np.ascontiguousarray(groups, dtype=np.int32)
    out = np.empty((L.shape[1], 5 + 3 * q.shape[1]))
    _check(load().b9h_group_influence_table(L.ctypes.data_as(_dp), L.shape[0], L.shape[1], q.ctypes.data_as(_dp), q.shape[1],
                                            g.ctypes.data_as(C.POINTER(C.c_int32)), len(g), out.ctypes.data_as(_dp)))
    return out


def _argv(prog, args):
    return (C.c_char_p * (len(args) + 1))(prog, *[str(a).encode() for a in args])


def influence_quantities(args, rows, log_post=None):
    """b9h_influence_quantities: (names, q [n_rows, Q], mean [Q], sd [Q]) as starInfluence forms them from `args` and the main-run
    rows [n_rows, B9_NPARAM] (log_post [n_rows] or None)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n = rows.shape[0]
    lp = None if log_post is None else np.ascontiguousarray(log_post, dtype=np.float64)
    names, q, mean, sd, nq = C.create_string_buffer(1024), np.empty(n * 12), np.empty(12), np.empty(12), C.c_int(0)
    _check(load().b9h_influence_quantities(len(args) + 1, _argv(b"starInfluence", args), rows.ctypes.data_as(_dp), lp.ctypes.data_as(_dp) if lp is not None else None,
                                           n, names, 1024, q.ctypes.data_as(_dp), mean.ctypes.data_as(_dp), sd.ctypes.data_as(_dp), C.byref(nq)))
    k = nq.value
    return names.value.decode().split(), q[:n * k].reshape(n, k).copy(), mean[:k].copy(), sd[:k].copy()


def influence_groups(args, ids, stage):
    """b9h_influence_groups: (names, ids [n_stars] int32) as starInfluence forms the groups from `args`, the catalogue's star ids
    and stages."""
    st = np.ascontiguousarray(stage, dtype=np.int32)
    names, g, ng = C.create_string_buffer(1024), np.full(len(ids), -1, np.int32), C.c_int(0)
    ip = C.POINTER(C.c_int32)
    _check(load().b9h_influence_groups(len(args) + 1, _argv(b"starInfluence", args), _names(ids), st.ctypes.data_as(ip), len(ids), names, 1024,
                                       g.ctypes.data_as(ip), C.byref(ng)))
    return names.value.decode().split(), g


def write_star_influence(path: str, ids, quantities, table) -> None:
    """b9h_write_star_influence: the .starInfluence file of a per-star table [len(ids), 4 + 3 len(quantities)]."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(len(ids), 4 + 3 * len(quantities))
    _check(load().b9h_write_star_influence(path.encode(), _names(ids), len(ids), _names(quantities), len(quantities), t.ctypes.data_as(_dp)))


def write_group_influence(path: str, groups, quantities, table) -> None:
    """b9h_write_group_influence: the .groupInfluence file of a per-group table [len(groups), 5 + 3 len(quantities)]."""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(len(groups), 5 + 3 * len(quantities))
    _check(load().b9h_write_group_influence(path.encode(), _names(groups), len(groups), _names(quantities), len(quantities), t.ctypes.data_as(_dp)))


def read_star_influence(path: str):
    """(ids, columns, table [n_stars, 4 + 3 Q]) of a .starInfluence file."""
    return read_table_file(path, "id")


def read_group_influence(path: str):
    """(groups, columns, table [G, 5 + 3 Q]) of a .groupInfluence file."""
    return read_table_file(path, "group")


def read_influence_scale(path: str):
    """(names, columns, table [Q, 2]: mean, sd) of an .influenceScale file."""
    return read_table_file(path, "name")


def star_influence_settings(args):
    """starInfluence's settings as the program parses `args` (flags, --config file): margIsoIncrem, nMassRatios, nPops, noGroups
    (ints), quantity (a list of names) and groupFile."""
    buf = C.create_string_buffer(4096)
    _check(load().b9h_star_influence_settings(len(args) + 1, _argv(b"starInfluence", args), buf, 4096))
    d = dict(line.split(" = ") if " = " in line else (line.rstrip(" ="), "") for line in buf.value.decode().splitlines())
    return dict(margIsoIncrem=int(d["margIsoIncrem"]), nMassRatios=int(d["nMassRatios"]), nPops=int(d["nPops"]), quantity=d["quantity"].split(),
                groupFile=d["groupFile"], noGroups=int(d["noGroups"]))
