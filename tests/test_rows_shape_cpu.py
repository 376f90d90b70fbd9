"""The row-group launch shape of the dense, window and pair kernels (csrc/tk_rows.h: units, rows a block, the reciprocal that
replaces the division, the grid) as a stand-alone sanitized program: tests/rows_shape_check.cpp calls the functions the launchers
and the kernels call, exhaustively over every units up to the tile."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shape_function_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rows_shape_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "rows_shape_check.cpp")])
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    word, n = r.stdout.decode().split()
    assert word == "ok" and int(n) > 2048 * 2048 // 2          # every unit index of every units was looked at
