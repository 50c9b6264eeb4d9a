"""What more than one test file needs: the error measure, engines loaded with tests/removal_cases.py's low-rank state, bit-for-bit
comparisons, the shared tolerances and inputs, host builds of kernel source, and the base of the stand-ins for the loaded library.
Import from here; do not copy.  Nothing of ekf_slam_amd is touched when this module is imported: CPU-only files import it on a
machine where no library is built."""
import ctypes
import os
import subprocess

import numpy as np

from removal_cases import lowrank_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-6                      # BASELINE.json's bar against the oracle
TOL_X32, TOL_KEPT32, TOL_ROW32 = 1e-9, 2e-9, 2e-7        # float tiles, DESIGN.md section 5, one step: x, entries of P kept in F64, a row
U2 = np.array([0.1, 1.0])       # the motion input and the correction's R of the GPU tests
R2 = np.diag([0.1, 0.2])
RPOS = np.array([[0.02, 0.005], [0.005, 0.03]])          # a position covariance with correlation
STORES_ALL = [(16, "f64"), (64, "f64"), (128, "f64"), (256, "f32"), (256, "f32_mixed"), (256, "f32_split")]


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def engine(mode="known", **kw):
    from ekf_slam_amd.engine import Engine
    return Engine(mode=mode, **kw)


def loaded(N, seed, mode="known", x=None, **kw):
    x0, s, d, U = lowrank_data(N, seed)
    e = engine(mode, **kw)
    e.load_lowrank_state(x0 if x is None else x, s, d, U)
    return e


def state(e):
    return e.get_x(), e.get_s(), e.get_P()


def getters(e):
    return [e.get_x(), e.get_s(), e.get_P(), e.get_P_diag_blocks(), e.digest()]


def blocks_of(P):
    n = P.shape[0]
    starts = np.concatenate([[0], np.arange(3, n, 2)])
    return np.array([P[a:a + 2, a:a + 2] for a in starts])


def assert_same(a, b, digest=True):
    assert a.N == b.N
    for get in ("get_x", "get_s", "get_P", "get_P_diag_blocks") + (("digest",) if digest else ()):
        np.testing.assert_array_equal(getattr(a, get)(), getattr(b, get)())


def check_state(e, ex, eP, storage, label, es=None):
    """x, P and the diagonal blocks of e (and N and s, where es is given) against the expectation, by the tolerances above; P
    symmetric as read."""
    x, s, P = state(e)
    blocks = e.get_P_diag_blocks()
    if es is not None:
        assert e.N == es.size
        np.testing.assert_array_equal(s, es)
    np.testing.assert_array_equal(P, P.T)
    n = ex.size
    kept = np.zeros((n, n), dtype=bool)                      # what float handles keep in F64
    kept[:3, :] = kept[:, :3] = True
    for a in range(3, n, 2):
        kept[a:a + 2, a:a + 2] = True
    scale = np.abs(eP).max()
    err_x, err_P, err_b = rel_err(x, ex), rel_err(P, eP), rel_err(blocks, blocks_of(eP))
    err_kept = float(np.abs(P - eP)[kept].max() / scale)
    err_row = float((np.abs(P - eP).max(axis=1) / np.abs(eP).max(axis=1)).max())
    print("%s [%s]: rel err x %.2e P %.2e blocks %.2e F64-kept %.2e worst row %.2e" % (label, storage, err_x, err_P, err_b, err_kept, err_row))
    if storage == "f64":
        assert err_x < REL and err_P < REL and err_b < REL
    else:
        assert err_x < TOL_X32 and err_kept < TOL_KEPT32 and err_b < TOL_KEPT32 and err_row <= TOL_ROW32


def status_of(fn):
    from ekf_slam_amd._lib import EkfError
    try:
        fn()
    except EkfError as ex:
        return ex.status, str(ex)
    return 0, ""


def run_ops(e, ops):
    """One predict and one append / measure / correct per operation of a continuation (merge_cases.continuation, for instance)."""
    for op in ops:
        e.predict(U2)
        if op[0] == "append":
            e.append(U2, R2, op[1], op[2])
        elif op[0] == "measure":
            e.measure(op[1], U2, op[2], op[3])
        else:
            e.correct(op[1], R2, op[2])


def same_npz(a, b):
    """Two .npz files hold the same arrays in the same order, name by name, dtype, shape and bytes (the zip container itself carries
    the time of writing, so the files are compared member by member)."""
    ga, gb = np.load(a), np.load(b)
    return ga.files == gb.files and all(ga[k].dtype == gb[k].dtype and ga[k].shape == gb[k].shape and ga[k].tobytes() == gb[k].tobytes()
                                        for k in ga.files)


# ------------------------------------------------------------------------------------------------------------------
# host builds of kernel source.  -mfma and -ffp-contract=off decide the bits that the "chain against singles, bit for bit" tests compare.
# ------------------------------------------------------------------------------------------------------------------
GXX = ["g++", "-std=c++17", "-I", os.path.join(ROOT, "ekf_slam_amd", "csrc")]
GXX_HOST = GXX + ["-O2", "-mfma", "-ffp-contract=off"]


def host_build(source_name, exe, flags=None):
    """tests/support/<source_name>.cpp built for the host as the program exe, with GXX_HOST -- or, for a build that has to name its own
    (a sanitizer build), with flags in place of GXX_HOST's -O2 -mfma -ffp-contract=off.  A failed build raises with the end of the
    compiler's stderr."""
    source = os.path.join(ROOT, "tests", "support", source_name + ".cpp")
    r = subprocess.run((GXX_HOST if flags is None else GXX + list(flags)) + [source, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def line_program(tmp_path_factory, source_name):
    """Builds tests/support/<source_name>.cpp; run(lines) feeds it the lines and returns one row of floats per line."""
    exe = host_build(source_name, str(tmp_path_factory.mktemp(source_name) / source_name))

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
        rows = [[float(v) for v in ln.split()] for ln in out.strip().split("\n")]
        assert len(rows) == len(lines)
        return rows
    return run


class RecorderBase:
    """Stand-in for the loaded library (no GPU here): what Engine needs to come up and to report an error.  A subclass adds the entry
    points it records and sets the two messages."""
    status_string = b"call not valid in the current state"
    last_error = b""

    def ekf_config_default(self, pcfg, mode):
        from ekf_slam_amd import _lib as L
        cfg = ctypes.cast(pcfg, ctypes.POINTER(L.EkfConfig)).contents
        cfg.mode, cfg.batch = mode, 1
        return 0

    def ekf_create(self, pcfg, ph):
        ctypes.cast(ph, ctypes.POINTER(ctypes.c_void_p)).contents.value = 0x1000
        return 0

    def ekf_destroy(self, h):
        return 0

    def ekf_status_string(self, rc):
        return self.status_string

    def ekf_last_error(self, h):
        return self.last_error
