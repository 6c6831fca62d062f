"""bench.py's command line outside a launcher: `python bench.py --gpus N` (N > 1) with no
torch.distributed environment starts itself under torch.distributed.run as a child process (one
rank per GPU, rendezvous on 127.0.0.1, the same arguments) and exits with the child's code."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_without_launcher_starts_torchrun_child(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    calls = []
    monkeypatch.setattr(subprocess, "call", lambda cmd: calls.append(cmd) or 7)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "8", "--warmup", "2"])
    assert bench.main() == 7
    (cmd,) = calls
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert any(c.startswith("--master-port=") for c in cmd)
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "8", "--warmup", "2"]


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    """`bench.py --gpus 1 --steps N --warmup W` is the plain run: --full (every pass beside the timed
    loop) and --dump-outputs are off unless given, and --steps is the timed frame count."""
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 20, 5)
    assert sum(bench.batch_sizes(a.steps, a.batch)) == 20
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "d")


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float32 (pixels, 4) files; a frame within its share whole, a larger one as the
    same sorted pixel sample in every run; all files together within 64 MB."""
    sys.path.insert(0, ROOT)
    import numpy as np

    import bench

    rng = np.random.default_rng(1)
    small = rng.integers(0, 256, (48, 64, 4), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), [("one", small), ("two", small[::-1])])
    one = np.load(tmp_path / "a" / "one.npy")
    assert one.dtype == np.float32 and np.array_equal(one, small.reshape(-1, 4).astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "two.npy"), small[::-1].reshape(-1, 4).astype(np.float32))

    big = np.arange(1920 * 1080 * 4, dtype=np.uint32).astype(np.uint8).reshape(1080, 1920, 4)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), [("first", big), ("last", big)])
    total = 0
    for name in ("first", "last"):
        x, y = np.load(tmp_path / "b" / (name + ".npy")), np.load(tmp_path / "c" / (name + ".npy"))
        total += os.path.getsize(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float32 and x.shape[1] == 4 and x.shape[0] < 1920 * 1080
        assert np.array_equal(x, y)
    assert total <= 64 * 1000 * 1000


def test_traffic_counts_the_product_kernels_only():
    """The HBM traffic pass sums the uninstrumented tracescreen launch: the STATS instantiations are
    recognised by their template argument (k_trace<L, STATS>, k_camerarays_group<STATS, ...>), not by
    the word `true` anywhere in the name."""
    sys.path.insert(0, ROOT)
    import bench

    assert bench.instrumented_kernel("k_trace<0, true>")
    assert bench.instrumented_kernel("k_trace<3, true>")
    assert bench.instrumented_kernel("k_camerarays_group<true, 512, 8>")
    assert not bench.instrumented_kernel("k_trace<0, false>")
    assert not bench.instrumented_kernel("k_trace<0, false, true>")  # a later template flag is not STATS
    assert not bench.instrumented_kernel("k_camerarays_group<false, 512, 4>")
    assert not bench.instrumented_kernel("k_finish")
