"""The ragged-table helper every host-buffer twin rebases its offsets with (csrc/po_hostbuf.h), as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer: tools/hostbuf_check.cpp has the cases and the expected values."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_helper_under_sanitizers(tmp_path):
    exe = str(tmp_path / "hostbuf_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "hostbuf_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
