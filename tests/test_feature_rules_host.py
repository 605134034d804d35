"""CPU: the feature / mode matrix of csrc/vct_feature_rules.h -- every subset of the features against every subset of the
modes, against the matrix written out in tests/feature_rules_check_main.cpp -- in a stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_feature_rules_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "feature_rules_check")
    src = os.path.join(ROOT, "tests", "feature_rules_check_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "feature_rules_check ok: 32768 cases" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
