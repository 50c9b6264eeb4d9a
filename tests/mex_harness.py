"""The MEX gateway (matlab/ekfslam_mex.c) compiled with ASan + UBSan against the mock of tests/support/mex_mock/ and run as a program
of its own; what every `*_cpu.py` file that drives one gateway command needs.  A test file keeps, as C text, its recording stand-in for
the entry point and the body of its driver's main between create and destroy; the rest is here.  Import from here; do not copy."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "support", "mex_mock")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "support", "mex_api_subset"), "-I", MOCK]
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
GATEWAY = [os.path.join(ROOT, "matlab", "ekfslam_mex.c"), os.path.join(MOCK, "mex_mock.c"), os.path.join(MOCK, "abi_stub.c")]


def build_and_run(files, exe):
    """The gateway, the mock, the stand-in library and files as one program; returns the lines it printed."""
    r = subprocess.run(GCC + INCLUDES + GATEWAY + files + ["-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, "the gateway misbehaved under the mock:\n" + r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def transcript_of(d, *sources):
    """Writes each C text into the directory d, builds them with the gateway and returns the transcript."""
    files = []
    for k, text in enumerate(sources):
        files.append(str(d / ("source%d.c" % k)))
        open(files[-1], "w").write(text)
    return build_and_run(files, str(d / "drv"))


def prelude(show=""):
    """What stands in front of a driver's main: call() prints `MEX <what> nrhs=<n> -> ok`, then whatever the C text show prints about
    out[0] and out[1], or `MEX ... -> ERROR <id> | <message>` and returns 1."""
    return r'''
#include <setjmp.h>
#include <stdio.h>
#include "ekfslam.h"
#include "mex_mock.h"
void arm_failure(void);
static mxArray *out[4];
static int call(const char *what, int nlhs, int nrhs, const mxArray **prhs) {
    out[0] = 0; out[1] = 0;
    if (setjmp(mock_err_jmp)) { printf("MEX %s nrhs=%d -> ERROR %s | %s\n", what, nrhs, mock_err_id, mock_err_msg); return 1; }
    mexFunction(nlhs, out, nrhs, prhs);
    printf("MEX %s nrhs=%d -> ok", what, nrhs);
''' + show + r'''    printf("\n");
    return 0;
}
#define D1(v) mock_double(1, 1, (const double[]){ v })
'''


PRELUDE = prelude()
PRELUDE_SHOWN = prelude(r'''    for (int k = 0; k < 2; ++k)
        if (out[k] && mxGetClassID(out[k]) != mxUINT64_CLASS) {
            printf(" out%d=%zux%zu[", k, mxGetM(out[k]), mxGetN(out[k]));
            for (size_t i = 0; i < mxGetM(out[k]) * mxGetN(out[k]); ++i) printf(i ? ",%g" : "%g", mxGetPr(out[k])[i]);
            printf("]");
        }
''')                              # ` out0=MxN[...]`, and ` out1=...` where the command was asked for a second output

OPEN = r'''int main(void) {
    const mxArray *cr[3] = { mock_string("create"), D1(1), D1(64) };
    if (call("create", 1, 3, cr)) return 1;
    const mxArray *h = out[0];
'''
OPEN_SILENT = r'''int main(void) {
    const mxArray *cr[3] = { mock_string("create"), D1(1), D1(64) };
    out[0] = 0;
    if (setjmp(mock_err_jmp)) return 1;
    mexFunction(1, out, 3, cr);
    const mxArray *h = out[0];
'''
CLOSE = r'''    const mxArray *de[2] = { mock_string("destroy"), h };
    if (call("destroy", 0, 2, de)) return 1;
    printf("LOCKS %d\nMISUSE %d\n", mock_lock_count, mock_misuse);
    return 0;
}
'''


def driver(body, head=PRELUDE, open_with=OPEN):
    """A whole driver: create, the C text body (which has the handle as `h`), destroy, the LOCKS and MISUSE lines."""
    return head + open_with + body + CLOSE


def driver_without(refused, open_with=OPEN):
    """The driver for a gateway linked against a library that lacks a symbol: create, the C text refused (calls that must fail with
    "this libekfslam has no ..."), a predict that must still work, destroy."""
    return driver(refused + r'''    const mxArray *pr[3] = { mock_string("predict"), h, mock_double(2, 1, (const double[]){ 0.1, 3 }) };
    if (call("predict", 1, 3, pr)) return 1;
''', open_with=open_with)
