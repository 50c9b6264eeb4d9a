"""CPU: the MEX gateway's `observe_model` command under the MEX mock with a recording stand-in for ekf_observe_model, the gateway
linked against a stand-in that lacks the symbol, and the MATLAB methods that forward to the command."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "support", "mex_mock")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "support", "mex_api_subset"), "-I", MOCK]
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_observe_model(ekf_handle *h, const ekf_model_obs *o, ekf_linear_result *res) {
    printf("ABI ekf_observe_model model=%d reserved=%d z=%g,%g R=%g,%g,%g,%g lm=%lld,%lld anchor=%g,%g gate=%g wait=%d\n", (int)o->model, (int)o->reserved,
           o->z[0], o->z[1], o->R[0], o->R[1], o->R[2], o->R[3], (long long)o->lm[0], (long long)o->lm[1], o->anchor[0], o->anchor[1], o->gate, res != 0);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    if (res) { res->nu[0] = 0.5; res->nu[1] = -0.25; res->S[0] = 1; res->S[1] = 2; res->S[2] = 3; res->S[3] = 4; res->d2 = 1.5; res->outcome = EKF_LINEAR_GATED; }
    return EKF_OK;
}
'''

_DRIVER = r'''
#include <setjmp.h>
#include <stdio.h>
#include "ekfslam.h"
#include "mex_mock.h"
void arm_failure(void);
static mxArray *out[4];
static int call(const char *what, int nlhs, int nrhs, const mxArray **prhs) {
    out[0] = 0;
    if (setjmp(mock_err_jmp)) { printf("MEX %s nrhs=%d -> ERROR %s | %s\n", what, nrhs, mock_err_id, mock_err_msg); return 1; }
    mexFunction(nlhs, out, nrhs, prhs);
    printf("MEX %s nrhs=%d -> ok", what, nrhs);
    if (out[0] && mxGetClassID(out[0]) != mxUINT64_CLASS) {
        printf(" out0=%zux%zu[", mxGetM(out[0]), mxGetN(out[0]));
        for (size_t i = 0; i < mxGetM(out[0]) * mxGetN(out[0]); ++i) printf(i ? ",%g" : "%g", mxGetPr(out[0])[i]);
        printf("]");
    }
    printf("\n");
    return 0;
}
#define D1(v) mock_double(1, 1, (const double[]){ v })
int main(void) {
    const mxArray *cr[3] = { mock_string("create"), D1(1), D1(64) };
    if (call("create", 1, 3, cr)) return 1;
    const mxArray *h = out[0];
    const mxArray *z = mock_double(2, 1, (const double[]){ 7, 8 }), *R = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    const mxArray *lm1 = D1(5), *lm2 = mock_double(2, 1, (const double[]){ 5, 3 }), *none = mock_double(0, 0, 0);
    const mxArray *anchor = mock_double(2, 1, (const double[]){ 10, -4 });
    /* range and bearing to landmark 5 (1-based), no wait */
    const mxArray *rb[9] = { mock_string("observe_model"), h, D1(1), z, R, lm1, none, D1(9.5), D1(0) };
    if (call("observe_model", 1, 9, rb)) return 1;
    /* the range to an anchor, the result waited for */
    const mxArray *an[9] = { mock_string("observe_model"), h, D1(2), mock_double(2, 1, (const double[]){ 7.5, 0 }), mock_double(2, 2, (const double[]){ 0.5, 0, 0, 0 }),
                             none, anchor, D1(1.0 / 0.0), D1(1) };
    if (call("observe_model anchor", 1, 9, an)) return 1;
    /* the distance between landmarks 5 and 3 */
    const mxArray *lr[9] = { mock_string("observe_model"), h, D1(5), mock_double(2, 1, (const double[]){ 2.5, 0 }), mock_double(2, 2, (const double[]){ 0.1, 0, 0, 0 }),
                             lm2, none, D1(4), D1(0) };
    if (call("observe_model pair", 1, 9, lr)) return 1;
    const mxArray *bad[9];
    for (int q = 0; q < 9; ++q) bad[q] = rb[q];
    if (!call("observe_model", 1, 8, rb)) return 1;
    bad[5] = mock_double(3, 1, (const double[]){ 1, 2, 3 });
    if (!call("observe_model three", 1, 9, bad)) return 1;
    bad[5] = lm1; bad[6] = anchor;
    if (!call("observe_model both", 1, 9, bad)) return 1;
    bad[5] = none; bad[6] = none;
    if (!call("observe_model neither", 1, 9, bad)) return 1;
    bad[6] = mock_double(3, 1, (const double[]){ 1, 2, 3 });
    if (!call("observe_model anchor3", 1, 9, bad)) return 1;
    bad[5] = D1(1.5); bad[6] = none;
    if (!call("observe_model frac", 1, 9, bad)) return 1;
    bad[5] = lm1; bad[4] = mock_double(2, 1, (const double[]){ 1, 2 });
    if (!call("observe_model badr", 1, 9, bad)) return 1;
    bad[4] = R; bad[3] = D1(1);
    if (!call("observe_model badz", 1, 9, bad)) return 1;
    bad[3] = z; bad[1] = D1(1);
    if (!call("observe_model noh", 1, 9, bad)) return 1;
    arm_failure();
    if (!call("observe_model", 1, 9, rb)) return 1;
    const mxArray *de[2] = { mock_string("destroy"), h };
    if (call("destroy", 0, 2, de)) return 1;
    printf("LOCKS %d\nMISUSE %d\n", mock_lock_count, mock_misuse);
    return 0;
}
'''

_DRIVER_WITHOUT = r'''
#include <setjmp.h>
#include <stdio.h>
#include "ekfslam.h"
#include "mex_mock.h"
static mxArray *out[4];
static int call(const char *what, int nrhs, const mxArray **prhs) {
    out[0] = 0;
    if (setjmp(mock_err_jmp)) { printf("MEX %s nrhs=%d -> ERROR %s | %s\n", what, nrhs, mock_err_id, mock_err_msg); return 1; }
    mexFunction(1, out, nrhs, prhs);
    printf("MEX %s nrhs=%d -> ok\n", what, nrhs);
    return 0;
}
#define D1(v) mock_double(1, 1, (const double[]){ v })
int main(void) {
    const mxArray *cr[3] = { mock_string("create"), D1(1), D1(64) };
    if (call("create", 3, cr)) return 1;
    const mxArray *h = out[0];
    const mxArray *ob[9] = { mock_string("observe_model"), h, D1(2), mock_double(2, 1, 0), mock_double(2, 2, 0), D1(1), mock_double(0, 0, 0), D1(1), D1(0) };
    if (!call("observe_model", 9, ob)) return 1;
    const mxArray *pr[3] = { mock_string("predict"), h, mock_double(2, 1, (const double[]){ 0.1, 3 }) };
    if (call("predict", 3, pr)) return 1;
    const mxArray *de[2] = { mock_string("destroy"), h };
    if (call("destroy", 2, de)) return 1;
    printf("LOCKS %d\nMISUSE %d\n", mock_lock_count, mock_misuse);
    return 0;
}
'''


def _build_and_run(files, exe):
    r = subprocess.run(GCC + INCLUDES + [os.path.join(ROOT, "matlab", "ekfslam_mex.c"), os.path.join(MOCK, "mex_mock.c"),
                                         os.path.join(MOCK, "abi_stub.c")] + files + ["-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, "the gateway misbehaved under the mock:\n" + r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def test_mex_gateway_marshals_a_model_observation_once(tmp_path):
    stub, drv = tmp_path / "model_stub.c", tmp_path / "model_drv.c"
    stub.write_text(_STUB)
    drv.write_text(_DRIVER)
    t = _build_and_run([str(stub), str(drv)], str(tmp_path / "drv"))
    # MATLAB's lm = 5 arrives 0-based once, R column-major as MATLAB holds it; no result asked for: an empty output
    i = t.index("ABI ekf_observe_model model=1 reserved=0 z=7,8 R=4,1,1,9 lm=4,-1 anchor=0,0 gate=9.5 wait=0")
    assert t[i + 1] == "MEX observe_model nrhs=9 -> ok out0=0x0[]"
    i = t.index("ABI ekf_observe_model model=2 reserved=0 z=7.5,0 R=0.5,0,0,0 lm=-1,-1 anchor=10,-4 gate=inf wait=1")
    assert t[i + 1] == "MEX observe_model anchor nrhs=9 -> ok out0=1x8[0.5,-0.25,1,2,3,4,1.5,2]"
    i = t.index("ABI ekf_observe_model model=5 reserved=0 z=2.5,0 R=0.1,0,0,0 lm=4,2 anchor=0,0 gate=4 wait=0")
    assert t[i + 1] == "MEX observe_model pair nrhs=9 -> ok out0=0x0[]"
    assert any(ln.startswith("MEX observe_model nrhs=8 -> ERROR ekfslam:usage") and "needs 9 arguments" in ln for ln in t)
    for which, what in (("three", "at most two landmarks"), ("both", "a landmark (anchor empty) or an anchor"), ("neither", "a landmark (anchor empty) or an anchor"),
                        ("anchor3", "an anchor of 2 elements"), ("frac", "whole numbers"), ("badr", "R needs 2 x 2 elements"), ("badz", "z needs 2 elements")):
        assert any(ln.startswith("MEX observe_model %s nrhs=9 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX observe_model noh nrhs=9 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_observe_model") for ln in t) == 4          # the three good calls and the injected failure
    assert "MEX observe_model nrhs=9 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    drv = tmp_path / "without_drv.c"
    drv.write_text(_DRIVER_WITHOUT)
    t = _build_and_run([str(drv)], str(tmp_path / "drv"))
    assert any(ln.startswith("MEX observe_model ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_observe_model" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_methods_forward_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+res\s*=\s*observeModel\(h,\s*model,\s*z,\s*R,\s*lm,\s*anchor,\s*gate,\s*wait\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('observe_model'," in m.group(1)
    for name, inner in (("observeRangeBearing", r"h\.observeModel\(1,\s*z,\s*R,\s*i,\s*\[\],"), ("observeRange", r"h\.observeModel\(2,\s*\[r 0\],\s*\[variance 0; 0 0\],\s*i,\s*\[\],"),
                        ("observeBearing", r"h\.observeModel\(3,\s*\[deg 0\],\s*\[variance 0; 0 0\],\s*i,\s*\[\],"), ("observeRelativeXY", r"h\.observeModel\(4,\s*z,\s*R,\s*i,\s*\[\],"),
                        ("observeLandmarkRange", r"h\.observeModel\(5,\s*\[dist 0\],\s*\[variance 0; 0 0\],\s*\[i j\],\s*\[\],"),
                        ("observeAnchorRange", r"h\.observeModel\(2,\s*\[r 0\],\s*\[variance 0; 0 0\],\s*\[\],\s*pos,"),
                        ("observeAnchorBearing", r"h\.observeModel\(3,\s*\[deg 0\],\s*\[variance 0; 0 0\],\s*\[\],\s*pos,")):
        m = re.search(r"function\s+res\s*=\s*%s\((.*?)\n        end\b" % name, text, re.S)
        assert m and re.search(inner, m.group(1)), name
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "observe_model")' in src and "#pragma weak ekf_observe_model" in src
