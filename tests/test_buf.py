"""DevBuf (nbldpc_amd/csrc/nbl_buf.h), the one owner of the host layer's device and pinned allocations, as a stand-alone program
(tests/buf_check.cpp) under the host's AddressSanitizer and UBSan.  No GPU is needed: without one every allocation fails and the
program checks the failure contract (nothing held, a text, the same again, release and destruction harmless); with one it checks
the growth contract (exact sizes, a smaller request keeps the buffer, a larger one replaces it, release leaves nothing)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "buf_check")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "nbldpc_amd", "csrc"), "buf_check", "BUF_CHECK=" + exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] in ("ok fail", "ok grow"), (out.stdout, out.stderr[-2000:])
