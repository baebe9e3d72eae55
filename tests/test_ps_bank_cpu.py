"""csrc/kernels/ps_bank.h (the hosted-PS bank and the optimizer spec of the native runtimes) as a
stand-alone host program, csrc/kernels/tests/ps_bank_check.cpp, built with AddressSanitizer +
UndefinedBehaviorSanitizer and run directly: no GPU, nothing loaded into Python.

a. OptimSpec::step_at under its two operand-width conventions, bit for bit against the two Python
   expectations of tests/test_numerics_cpu.py::test_native_adam_step_size_matches_python_bitwise:
   true doubles (ops/adam.py adam_coeffs) and float32 hyper-parameters widened to double.
b. PsBank: refusals, advance() from two threads, t / set_t, record(), lookup by PS id.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from ddl_amd.ops.adam import AdamHyper, adam_coeffs

ADAM, MOMENTUM = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "distributed-deep-learning_amd", "csrc", "kernels", "tests",
                   "ps_bank_check.cpp")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("ps_bank") / "ps_bank_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-pthread", SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def _run(exe, mode, stdin=""):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, mode], input=stdin, capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _bits(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def test_step_sizes_bitwise(check_exe):
    f32 = lambda x: float(np.float32(x))
    ts = (1, 2, 3, 10, 1000, 100000)
    hypers = [(lr, 0.9, 0.999) for lr in (1e-4, 3e-3, 0.1)] + [(1e-4, 0.5, 0.75)]
    rows, want = [], []
    for lr, b1, b2 in hypers:
        h = AdamHyper(lr=lr, beta1=b1, beta2=b2)
        lr32, b132, b232 = f32(lr), f32(b1), f32(b2)
        for t in ts:
            widened = lr32 * math.sqrt(1.0 - b232 ** t) / (1.0 - b132 ** t)
            rows += [("f64", lr, b1, b2, ADAM, t), ("f32", lr, b1, b2, ADAM, t),
                     ("f64", lr, b1, b2, MOMENTUM, t), ("f32", lr, b1, b2, MOMENTUM, t)]
            want += [_bits(adam_coeffs(h, t)), _bits(widened), _bits(lr), _bits(lr)]
    assert f32(0.5) == 0.5 and f32(0.75) == 0.75  # (the pair that is exact in float32)
    text = "".join("%s %r %r %r %d %d\n" % r for r in rows)
    got = _run(check_exe, "steps", text).split()
    assert len(got) == len(rows)
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
    assert not bad, bad[:8]
    # the two conventions are different operands (1e-4 and 0.999 are no float32 values): they
    # must part on some row of this table, or the comparison above shows nothing about the width
    adam = [i for i, r in enumerate(rows) if r[4] == ADAM]
    differ = [rows[i][1:] for i in adam[::2] if got[i] != got[i + 1]]
    print("Adam rows on which the conventions differ: %d of %d" % (len(differ), len(adam) // 2))
    assert differ


def test_bank(check_exe):
    assert _run(check_exe, "bank").startswith("OK ")
