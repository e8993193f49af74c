"""The C++ body wrappers (include/s3hash_batch.hpp namespace s3h): the AWS documentation's example
framed by s3h::chunk_body_host, its two known lengths and the argument errors, in a program built
by `make cpptests` (tests/cpp/chunk_body_wrappers_test.cpp).  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_wrappers_known_answer():
    subprocess.run(["make", "-C", ROOT, "cpptests"], check=True, capture_output=True)
    exe = os.path.join(ROOT, "tests", "cpp", "build", "chunk_body_wrappers_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
