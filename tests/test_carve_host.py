"""CPU: csrc/lzx_carve.h, the layout lists of the graph routines' arenas, on a host buffer.  tests/carve_check.cc is a program of
its own: it is compiled here with the host compiler of host/Makefile and -fsanitize=address,undefined and run as a child process
(nothing of it is loaded into this interpreter).  It walks the shapes of list the call sites use -- u32 pieces of lzx_even(n)
words before u64 ones, the five conditional pieces of lzx_paths.hip in all 32 combinations, raw bytes behind a 256-byte boundary --
over a malloc of exactly the counted bytes and writes every piece to its end: an overrun is AddressSanitizer's finding, a piece
off its alignment UBSan's, and both end the program with a status other than 0."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msc-hpc-final-project_amd", "csrc")


def test_the_carver_on_a_host_buffer(tmp_path):
    assert shutil.which("g++"), "g++, the host compiler of host/Makefile, is not installed"
    exe = str(tmp_path / "carve_check")
    # -static-libasan / -static-libubsan: with the runtimes inside the program it does not depend on ASan's check that its shared
    # runtime comes first among the loaded libraries; -fno-sanitize-recover: a finding of UBSan ends the program, as ASan's do
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "carve_check.cc"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("carve ok")


def test_the_header_stands_alone():
    """host only: nothing of HIP and nothing of the project is included, so that a plain C++ program can include it"""
    with open(os.path.join(CSRC, "lzx_carve.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(inc in ("<cstddef>", "<cstdint>") for inc in includes), includes
