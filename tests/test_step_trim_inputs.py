"""CPU checks behind tests/test_gpu_step_trim.py: its pow input set reaches both paths of
pow_nonneg_wave, and on that set the oracle's ro_pow equals rt_math.h's pow_nonneg built for the host."""
import os
import subprocess

import numpy as np

import oracle_lib as O
from test_gpu_step_trim import wave_pow_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST_POW = r"""
#include "rt_math.h"
#include <stdio.h>
int main(int argc, char** argv)
{
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    float v[2];
    while (fread(v, 4, 2, in) == 2) {
        float r[2] = {rtm::pow_nonneg(v[0], v[1]), rtm::pow_nonneg_wave(v[0], v[1])};
        fwrite(r, 4, 2, out);
    }
    fclose(out);
    return 0;
}
"""


def test_wave_pow_inputs_reach_both_paths():
    """Waves 0..31: every y*log2(x) inside [-150, 128) and no zero base; waves 32..63: exactly one lane
    with a zero or denormal base or an argument outside the range (by the oracle's own log2)."""
    x, y = wave_pow_inputs()
    assert x.size == 4096 and x.dtype == np.float32 and y.dtype == np.float32
    a = (y * O.unary(1, x)).astype(np.float32).reshape(64, 64)
    xs = x.reshape(64, 64)
    out = ~((a >= -150) & (a < 128))
    assert not out[:32].any() and np.all(xs[:32] >= 1e-6)
    odd = out | (xs < np.float32(1.1754944e-38))
    assert np.all(odd[32:].sum(axis=1) == 1)
    assert out[32:].any(axis=1).sum() >= 16 and (xs[32:] == 0).any(axis=1).sum() >= 6
    assert {float(v) for v in a.ravel() if v in (-150.0, 128.0)} == {-150.0, 128.0}
    m = x.view(np.uint32) & 0x007FFFFF
    assert ((m > 0x3504F3) & (m <= 0x3504F5)).any() and ((m < 0x3504F3) & (m >= 0x3504F1)).any() and (m == 0x3504F3).any()


def test_oracle_pow_equals_host_pow_nonneg(tmp_path):
    x, y = wave_pow_inputs()
    src, exe = tmp_path / "host_pow.cpp", tmp_path / "host_pow"
    src.write_text(HOST_POW)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    "-o", str(exe), str(src)], check=True)
    np.stack([x, y], axis=1).astype(np.float32).tofile(tmp_path / "in.bin")
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 2)
    ref = O.binary(0, x, y)
    assert np.array_equal(got[:, 0].view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(got[:, 1].view(np.uint32), ref.view(np.uint32))
