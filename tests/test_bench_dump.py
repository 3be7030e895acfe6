"""bench.py --dump-outputs / --full: the dump helper on host tensors (no GPU), and one plain run of
the benchmark at a small size whose dumped arrays are checked against the oracle's file and the
input image (the decode is lossless, so the decoded sample is a sample of the input)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _positions(bench, B, img):
    """the sample positions dump_outputs draws for B images of img bytes: (u, pos)"""
    rng = np.random.default_rng(bench.DUMP_SEED)
    u = rng.random(max(1, bench.DUMP_FILE_SAMPLES // B))
    return u, rng.integers(0, img, min(img, max(1, bench.DUMP_IMAGE_SAMPLES // B)))


def test_dump_outputs_host(tmp_path):
    import torch
    import bench
    B, stride, img = 3, 1000, 3000
    g = torch.Generator().manual_seed(5)
    out = torch.randint(0, 256, (B * stride,), dtype=torch.uint8, generator=g)
    dec = torch.randint(0, 256, (B * img,), dtype=torch.uint8, generator=g)
    sizes = [1000, 1, 0]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch, out, stride, sizes, dec, img, prefix="p_")
    arrs = {}
    for n in ("file_sizes", "file_bytes_sample", "decoded_sample"):
        a, b = np.load(tmp_path / "a" / ("p_%s.npy" % n)), np.load(tmp_path / "b" / ("p_%s.npy" % n))
        assert np.array_equal(a, b), n
        arrs[n] = a
    assert arrs["file_sizes"].dtype == np.float64 and arrs["file_sizes"].tolist() == [1000.0, 1.0, 0.0]
    u, pos = _positions(bench, B, img)
    fs, ds = arrs["file_bytes_sample"], arrs["decoded_sample"]
    assert fs.dtype == np.float32 and fs.shape == (B, u.size) and ds.dtype == np.float32 and ds.shape == (B, pos.size)
    o, d = out.numpy(), dec.numpy()
    assert np.array_equal(fs[0], o[:1000][(u * 1000).astype(np.int64)])
    assert np.all(fs[1] == o[stride]) and not fs[2].any()          # a 1-byte file, an empty file
    for b in range(B):
        assert np.array_equal(ds[b], d[b * img:(b + 1) * img][pos])
    # the 64 MB budget of --dump-outputs, whatever the batch
    assert 4 * (bench.DUMP_FILE_SAMPLES + bench.DUMP_IMAGE_SAMPLES) + 8 * 4096 <= 64 * 1000 * 1000


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path, orc):
    import bench
    from hoh_ans import synth
    W, D, B, K, seed, noise = 512, 2, 2, 4, 1, 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
                        "--size", str(W), "--inflight", str(D), "--batch", str(B), "--seed", str(seed),
                        "--noise", str(noise), "--dump-outputs", str(tmp_path / "dump")],
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == K and res["warmup"] == 1 and res["unit"] == "MB/s" and res["higher_is_better"] is True
    assert res["dtype"] == "u8" and res["ms_per_step"] > 0 and res["detail"]["lossless"] is True
    assert res["value"] == pytest.approx(W * W * 3 * B / res["ms_per_step"] / 1e3, rel=1e-3)
    # a plain run carries none of what --full adds
    assert "roofline" not in res and "cpu_baseline" not in res
    assert not {"file_sha256", "single_image_MBps", "no_index_pipeline_MBps", "config2_single_stream",
                "pmc_hbm_bytes_per_launch"} & set(res["detail"])
    # step K - 1 ran on slot (K - 1) % D, whose images are seeds seed + slot * B ...
    slot = (K - 1) % D
    sizes = np.load(tmp_path / "dump" / "file_sizes.npy")
    fs = np.load(tmp_path / "dump" / "file_bytes_sample.npy")
    ds = np.load(tmp_path / "dump" / "decoded_sample.npy")
    u, pos = _positions(bench, B, W * W * 3)
    assert sizes.dtype == np.float64 and fs.dtype == np.float32 and ds.dtype == np.float32
    for b in range(B):
        img = synth.synth_rgb(W, W, seed=seed + slot * B + b, noise=noise)
        want, _ = orc.choh(img)
        assert sizes[b] == len(want)
        assert np.array_equal(fs[b], np.frombuffer(want, np.uint8)[(u * len(want)).astype(np.int64)])
        assert np.array_equal(ds[b], img.reshape(-1)[pos])
