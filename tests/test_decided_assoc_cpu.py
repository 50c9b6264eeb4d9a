"""CPU: the surfaces of the device-decided branch (cfg.device_assoc = 4, include/ekfslam.h) that need no GPU -- the Python layer hands
the value to ekf_create, the MEX gateway's optional positional argument after pass_arith reaches cfg.device_assoc (the gateway
compiled against the MEX mock of tests/support/mex_mock/, with ekf_create wrapped to report the config), and the scan plans the
GPU tests use make the position-weighted likelihood reject signature matches."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mex_harness import INCLUDES, MOCK, ROOT

_WRAP = r'''
#include <stdio.h>
#include "ekfslam.h"
int32_t stub_ekf_create(const ekf_config *cfg, ekf_handle **out);
int32_t ekf_create(const ekf_config *cfg, ekf_handle **out) {
    printf("CFG device_assoc=%d pass_arith=%d storage=%d\n", cfg->device_assoc, cfg->pass_arith, cfg->storage);
    return stub_ekf_create(cfg, out);
}
'''

_DRIVER = r'''
#include <setjmp.h>
#include <stdio.h>
#include "ekfslam.h"
#include "mex_mock.h"
#define D1(v) mock_double(1, 1, (const double[]){ v })
static int call(int nrhs, const mxArray **prhs) {
    mxArray *out[4] = { 0 };
    if (setjmp(mock_err_jmp)) { printf("ERROR %s\n", mock_err_msg); return 1; }
    mexFunction(1, out, nrhs, prhs);
    return 0;
}
int main(void) {
    const mxArray *a10[10] = { mock_string("create"), D1(1), D1(64), D1(256), D1(8), D1(0), D1(0), D1(1), D1(1), D1(1) };
    const mxArray *a11[11] = { mock_string("create"), D1(1), D1(64), D1(0), D1(8), D1(0), D1(0), D1(1), D1(0), D1(0), D1(4) };
    if (call(10, a10) || call(11, a11)) return 1;
    return 0;
}
'''


def test_mex_create_takes_device_assoc_after_pass_arith(tmp_path):
    wrap, drv, exe = tmp_path / "wrap.c", tmp_path / "drv.c", str(tmp_path / "drv")
    wrap.write_text(_WRAP)
    drv.write_text(_DRIVER)
    objs = []
    for src, extra in ((os.path.join(MOCK, "abi_stub.c"), ["-Dekf_create=stub_ekf_create"]), (os.path.join(MOCK, "mex_mock.c"), []),
                       (os.path.join(ROOT, "matlab", "ekfslam_mex.c"), []), (str(wrap), []), (str(drv), [])):
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        r = subprocess.run(["gcc", "-std=c99", "-c", "-Wall"] + extra + INCLUDES + [src, "-o", o], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        objs.append(o)
    r = subprocess.run(["gcc"] + objs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cfgs = [l for l in r.stdout.splitlines() if l.startswith("CFG ")]
    assert cfgs == ["CFG device_assoc=0 pass_arith=1 storage=1",      # (the stub's defaults; no 11th argument: left alone)
                    "CFG device_assoc=4 pass_arith=0 storage=0"]


def test_engine_hands_device_assoc_4_to_create(monkeypatch):
    """Engine(device_assoc=4) reaches ekf_create unchanged (a recording stand-in for the library: no GPU here)."""
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    seen = {}

    class FakeLib:
        def ekf_config_default(self, pcfg, mode):
            cfg = ctypes.cast(pcfg, ctypes.POINTER(L.EkfConfig)).contents
            cfg.mode, cfg.device_assoc, cfg.batch = mode, 3 if mode == L.EKF_MODE_UC else 0, 1
            return L.EKF_OK

        def ekf_create(self, pcfg, ph):
            cfg = ctypes.cast(pcfg, ctypes.POINTER(L.EkfConfig)).contents
            seen.update(device_assoc=cfg.device_assoc, w_pos=cfg.w_pos, mode=cfg.mode)
            return L.EKF_ERR_NO_DEVICE

        def ekf_status_string(self, rc):
            return b"no device"

        def ekf_last_error(self, h):
            return b""

    monkeypatch.setattr(L, "lib", lambda: FakeLib())
    with pytest.raises(L.EkfError):
        E.Engine(mode="uc", capacity=16, device_assoc=4, w_pos=1.0)
    assert seen == {"device_assoc": 4, "w_pos": 1.0, "mode": L.EKF_MODE_UC}


def test_plans_make_the_position_cost_reject_signature_matches(oracle_lib):
    from decided_plans import make_plan, oracle_run
    from oracle.ekf_structured import StructuredEKF
    plan = make_plan(7, 400, 30, 8)
    ref = StructuredEKF(400, "uc", Rc=(0.01, 0.01), w_pos=1.0, s_thresh=0.5)
    assert oracle_run(ref, plan) >= 10
    # some scan corrects a landmark it appended itself, and some scan's appends cross an edge of 16 rows
    assert any(len(set(rows[:, 2])) < len(rows) for _, rows, _, _ in plan[1:])
    assert np.isfinite(ref.x).all()
