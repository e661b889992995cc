"""The block-layout cursor and the layout of a relocalization batch's inputs (ptz-calib_amd/csrc/ptz_block_layout.h,
ptz_krt_batch_layout.h), which the four host-form relocalization entry points share: compiled for the host on their own and checked by
tests/cpu_harness/krt_batch_layout_harness.cc, a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "krt_batch_layout_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpu_harness", "krt_batch_layout_harness.cc")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout
    assert int(r.stdout.split()[0]) == 5 * 8 * 5 * 4  # every combination was laid out
