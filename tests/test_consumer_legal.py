"""integration/c/consumer_legal.c without a GPU: the plain-C consumer of cattus_hip_apply_legal is strict C99, as consumer.c is
(test_integration_files.py); test_consumer_legal_gpu.py runs it."""

import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_c_consumer_legal_is_strict_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D_POSIX_C_SOURCE=200809L", f"-I{ROOT / 'include'}", "-c",
                           str(ROOT / "integration" / "c" / "consumer_legal.c"), "-o", str(tmp_path / "consumer_legal.o")])
