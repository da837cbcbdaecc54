"""What the tests of the command-line programs share (a plain module, next to golden_util.py): running a built program, reading
a .phot through the library, and the shared flag table's view of a command line."""
import ctypes as C
import os
import subprocess

import numpy as np

from base_amd import abi


def cli(name, *args, timeout=600):
    """Runs base_amd/host/bin/<name> with the arguments; -> the CompletedProcess (text, both streams captured)."""
    from base_amd import host_build
    return subprocess.run([os.path.join(host_build.BIN, name), *args], capture_output=True, text=True, timeout=timeout)


def read_phot(path):
    """A .phot file as b9h_read_phot reads it (no magnitude cut): the arrays of a b9_stars, as a dict."""
    from base_amd import hostlib
    lib = hostlib.load()
    h, view = C.c_void_p(), abi.b9_stars()
    buf = C.create_string_buffer(512)
    assert lib.b9h_read_phot(path.encode(), -1e300, 1e300, 0, C.byref(h), C.byref(view), buf, 512) == 0, lib.b9h_last_error()
    n, nf = view.n_stars, view.n_filt
    g = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()     # noqa: E731
    d = dict(n_filt=nf, obs=g(view.obs, n * nf), sigma=g(view.sigma, n * nf), mass1=g(view.mass1, n), mass_ratio=g(view.mass_ratio, n),
             clust_prior=g(view.clust_prior, n), stage=g(view.stage, n), wd_type=g(view.wd_type, n),
             filter_prior_min=g(view.filter_prior_min, nf), filter_prior_max=g(view.filter_prior_max, nf))
    lib.b9h_free_phot(h)
    return d


def settings_dump(args):
    """b9h_settings_dump: the settings keys a command line sets through the SHARED flag table alone (no program's own flags), as
    a dict key -> value string.  Raises hostlib.HostError as the parser does."""
    from base_amd import hostlib
    lib = hostlib.load()
    argv = (C.c_char_p * (len(args) + 1))(b"prog", *[str(a).encode() for a in args])
    out = C.create_string_buffer(8192)
    if lib.b9h_settings_dump(len(args) + 1, argv, out, 8192) != 0:
        raise hostlib.HostError(lib.b9h_last_error().decode())
    return dict(line.split(" = ", 1) for line in out.value.decode().splitlines())
