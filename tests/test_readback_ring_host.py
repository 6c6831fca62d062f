"""CPU tests of the readback ring (rt_readback_*, rt_recorder_set_async): argument checks that need no device,
and the ring's host-only bookkeeping (gpgpuraytrace_amd/csrc/rt_ring.h) driven by a stand-alone C++ program under
AddressSanitizer + UBSan."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1


def test_null_and_bad_arguments_need_no_device():
    import gpgpuraytrace_amd as G
    L = G.lib()
    h = C.c_void_p(1)
    fake = C.c_void_p(0)  # (a null device: the format and depth checks come first)
    for fmt, depth, why in ((0, 0, b"1..8"), (0, 9, b"1..8"), (1, -1, b"1..8"), (2, 3, b"format"), (-1, 3, b"format")):
        assert L.rt_readback_create(fake, fmt, depth, C.byref(h)) == RT_ERR_INVALID
        assert why in L.rt_last_error(), (fmt, depth, L.rt_last_error())
        assert h.value is None
    assert L.rt_readback_create(None, 0, 3, C.byref(h)) == RT_ERR_INVALID and b"device" in L.rt_last_error()
    assert L.rt_readback_create(None, 0, 3, None) == RT_ERR_INVALID  # null out pointer
    t = C.c_ulonglong(7)
    assert L.rt_readback_submit(None, C.byref(t)) == RT_ERR_INVALID and t.value == 7
    assert L.rt_readback_ready(None, 0) == RT_ERR_INVALID
    p = C.c_void_p(1)
    assert L.rt_readback_wait(None, 0, C.byref(p)) == RT_ERR_INVALID and p.value is None
    assert L.rt_readback_release(None, 0) == RT_ERR_INVALID
    L.rt_readback_destroy(None)
    assert L.rt_recorder_set_async(None, 3) == RT_ERR_INVALID


def test_python_layer_exports_and_format_names():
    import gpgpuraytrace_amd as G
    assert "ReadbackRing" in G.__all__ and G.ReadbackRing.FORMATS == {"rgba8": 0, "bgrx": 1}
    with pytest.raises(ValueError):
        G.ReadbackRing(None, "rgb", 3)
    assert hasattr(G.Device, "readback_ring") and hasattr(G.Recorder, "set_async")


def test_ring_bookkeeping_under_sanitizers(tmp_path):
    """tests/tools/ring_check.cpp: fill, full, release and wrap-around over many more tickets than slots,
    out-of-order release, stale tickets, cancel.  Its own main, its own process: nothing of it is loaded into
    this interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/ring_check.cpp"
    exe = str(tmp_path / "ring_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "ring_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ring_check ok")
