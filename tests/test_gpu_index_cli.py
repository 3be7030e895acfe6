"""GPU: the sidecar flags of the CLIs -- `choh ... --index a.hix`, `dhoh ... --index a.hix`,
`dhoh ... --write-index b.hix`.  The sidecar choh writes and the one dhoh builds from the file
alone are the same bytes; without the flags both tools behave as before (tests/test_gpu_cli.py)."""
import os
import subprocess

import pytest

import oracle
from hoh_ans import natural, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hoh-ans_amd", "bin")
CHOH, DHOH = os.path.join(BIN, "choh"), os.path.join(BIN, "dhoh")


def _run(args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_sidecar_roundtrip(tmp_path):
    W, H = 768, 512
    img = synth.synth_rgb(W, H, seed=21, noise=4)
    src, hohf = tmp_path / "in.rgb", tmp_path / "o.hoh"
    src.write_bytes(img.tobytes())
    r = _run([CHOH, src, hohf, W, H, "-s0", "--index", tmp_path / "a.hix"])
    assert r.returncode == 0, r.stdout + r.stderr
    want, printed = oracle.choh(img)
    assert hohf.read_bytes() == want and int(r.stdout.strip().splitlines()[-1]) == printed
    a = (tmp_path / "a.hix").read_bytes()
    assert a[:4] == b"HOHX" and len(a) > 48
    r = _run([DHOH, hohf, tmp_path / "b1.rgb", "--index", tmp_path / "a.hix"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "b1.rgb").read_bytes() == img.tobytes()
    r = _run([DHOH, hohf, tmp_path / "b2.rgb", "--write-index", tmp_path / "b.hix"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "b2.rgb").read_bytes() == img.tobytes()
    assert (tmp_path / "b.hix").read_bytes() == a
    # a damaged sidecar is refused, a usage error with several devices
    (tmp_path / "c.hix").write_bytes(a[:-1])
    assert _run([DHOH, hohf, tmp_path / "b3.rgb", "--index", tmp_path / "c.hix"]).returncode == 7
    assert _run([DHOH, hohf, tmp_path / "b3.rgb", "--index", tmp_path / "a.hix", "--gpus", "2"]).returncode == 1
    assert _run([CHOH, src, hohf, W, H, "-s0", "--index", tmp_path / "d.hix", "--gpus", "2"]).returncode == 1


def test_sidecar_of_a_speed_file_is_empty(tmp_path):
    W, H = 512, 256
    img = natural.natural_rgb(W, H, seed=3)
    src, hohf = tmp_path / "in.rgb", tmp_path / "o.hoh"
    src.write_bytes(img.tobytes())
    r = _run([CHOH, src, hohf, W, H, "-s1", "--decodable", "--index", tmp_path / "a.hix"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert len((tmp_path / "a.hix").read_bytes()) == 48
    r = _run([DHOH, hohf, tmp_path / "b.rgb", "--write-index", tmp_path / "b.hix"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "b.rgb").read_bytes() == img.tobytes()
    assert (tmp_path / "b.hix").read_bytes() == (tmp_path / "a.hix").read_bytes()
    r = _run([DHOH, hohf, tmp_path / "c.rgb", "--index", tmp_path / "a.hix"])
    assert r.returncode == 0 and (tmp_path / "c.rgb").read_bytes() == img.tobytes()
