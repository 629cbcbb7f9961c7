"""The host-side planner of the dW launch and its optimizer (csrc/hip/tree_plan.h): split
plans, block geometry, segment layout, the fused-optimizer description (one TrOptCore copied
whole), the sampler-argument check of the three launches that carry a sampler (one case per
condition it rejects) and their rejections, checked on the CPU by csrc/tests/tree_plan_selftest.cc, a stand-alone program built with
AddressSanitizer + UBSan.  The plan numbers are the ones the GPU tests pin through the plans
(test_dw_opt_fuse.py, test_dw_route_pipe.py, test_dw_fold.py)."""
import os
import subprocess

from euler_amd import _build


def test_tree_plan_selftest_under_asan_ubsan():
    exe = _build.build_plan_selftest()
    env = dict(os.environ)
    # the environment may preload a library of its own: tolerate it rather than touch it
    env["ASAN_OPTIONS"] = "detect_leaks=1 halt_on_error=1 verify_asan_link_order=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1 print_stacktrace=1"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tree_plan_selftest OK" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
