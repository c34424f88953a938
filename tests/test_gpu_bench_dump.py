"""bench.py --dump-outputs and the plain / --full split.

  * dump_outputs on a small C4 shard (mixed lengths and commands, 1 frame in 16 corrupted, more
    packets than the sample so the seeded draw is used): every file equals the oracle's encode /
    decode of the sampled packets, in float32 / float64
  * a plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` run: K timed steps and
    ms_per_step on the line, none of the --full measurements, the files written and under 64 MB
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from rsock_amd import workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = b"hello135"
N = 5000
NAMES = ("packet_idx", "enc_status", "dec_status", "dec_hlen", "dec_cmd", "dec_id", "dec_conv", "dec_conn_key",
         "dec_pay_off", "dec_pay_len", "dec_n_valid", "dec_valid_idx", "frame_idx", "frames")


def test_dump_outputs_equals_oracle_on_the_sample(oracle, gpu, tmp_path, monkeypatch):
    import torch

    from rsock_amd.codec import Codec

    monkeypatch.setattr(bench, "DUMP_PACKETS", 1000)
    monkeypatch.setattr(bench, "DUMP_FRAMES", 100)
    d = workload.describe("c4", 0, N, n=N)
    w = workload.DeviceWorkload(d, gpu)
    cx = Codec(KEY, 0)
    try:
        cx.output_batch(w.payload, w.pay_off, w.pay_len, w.cmd, w.conv, w.conn_key, w.frame, w.frame_off,
                        w.status, id_uniform=workload.ID_UNIFORM, pad128=d.pad == 128)
        w.corrupt_frames()
        cx.onrecv_batch(w.frame, w.frame_off, w.frame_len, w.dec)
        torch.cuda.synchronize()
        shapes = bench.dump_outputs(torch, str(tmp_path), d, w)
    finally:
        cx.close()
    got = {k: np.load(tmp_path / f"{k}.npy") for k in NAMES}
    assert set(shapes) == set(NAMES) and all(list(got[k].shape) == shapes[k] for k in NAMES)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())

    frames, st = oracle.encode_batch(KEY, workload.payload_bytes_np(d), d, workload.ID_UNIFORM)
    for i in np.nonzero(d.corrupt)[0]:
        frames[int(d.frame_off[i])] ^= 1
    exp = oracle.decode_batch(KEY, frames, d.frame_off, d.frame_len)
    idx = got["packet_idx"].astype(np.int64)
    assert len(idx) == 1000 and np.array_equal(idx, bench.dump_sample(N, 1000, 0x5EED0001))
    assert np.array_equal(got["enc_status"], st[idx])
    for k in ("status", "hlen", "cmd", "conv", "pay_off", "pay_len"):
        assert np.array_equal(got[f"dec_{k}"], exp[k][idx].astype(np.float64)), k
    assert np.array_equal(got["dec_id"], exp["id"].reshape(-1, 8)[idx])
    ck = exp["conn_key"].view(np.uint64)[idx]
    assert np.array_equal(got["dec_conn_key"][:, 0], ck & np.uint64(0xFFFFFFFF))
    assert np.array_equal(got["dec_conn_key"][:, 1], ck >> np.uint64(32))
    nv = int(exp["n_valid"])
    assert got["dec_n_valid"].tolist() == [nv] and 0 < nv < N
    vi = np.where(idx < nv, exp["valid_idx"].astype(np.float64)[np.minimum(idx, nv - 1)], -1.0)
    assert np.array_equal(got["dec_valid_idx"], vi) and (vi < 0).any() and (vi >= 0).any()
    fidx = got["frame_idx"].astype(np.int64)
    assert np.array_equal(fidx, bench.dump_sample(N, 100, 0x5EED0002))
    # the oracle's arena has the same slots; the slot tail past the frame and its zero pad stays zero
    assert np.array_equal(got["frames"], frames.reshape(N, d.frame_pitch)[fidx])


def test_plain_run_times_k_steps_and_dumps(gpu, tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--config", "c2", "--packets", "8192", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["n_gpus"] == 1 and rec["unit"] == "Mpkt/s" and rec["dtype"] == "u8"
    assert rec["higher_is_better"] is True and rec["value"] > 0 and rec["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: packets x steps / time, and time / steps
    assert rec["value"] == pytest.approx(8192 / (rec["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    for k in ("cpu_baseline", "scale_n1_c5", "variant_tag_table_lut", "kernels_ms", "roofline"):
        assert k not in rec, k
    assert sorted(os.listdir(out)) == sorted(f"{k}.npy" for k in NAMES)
    assert rec["outputs"]["arrays"]["frames"] == [bench.DUMP_FRAMES, 96]
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) < 64e6
    a = np.load(out / "dec_n_valid.npy")
    assert a.dtype == np.float64 and a.tolist() == [8192.0]
