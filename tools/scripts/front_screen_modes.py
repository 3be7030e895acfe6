#!/usr/bin/env python3
"""Measurement (checking build): how k_front256's two-mode LZ screen spends its chunks on the bench
image and on the natural image -- the fraction of chunks the fast path passes with no flagged lane,
resolves lane by lane, and hands to table mode, and the mode switches per tile (EncodeJob::dbg
56..60).  Knobs HOH_F2_MLOG2 / HOH_F2_THR / HOH_F2_QUIET / HOH_F2_MODE apply.
    python3 tools/scripts/front_screen_modes.py [W=4096]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "hoh-ans_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hoh_ans  # noqa: E402
from checklib import CheckLib  # noqa: E402

W = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
c = CheckLib()
nt = (W // 256) ** 2
for name, rgb in (("bench synth_rgb(seed 1, noise 4)", hoh_ans.synth_rgb_dev(W, W, 1, 4)),
                  ("natural(seed 1)", c.natural(W, W, 1, torch))):
    torch.cuda.synchronize()
    c.encode(rgb.reshape(-1), W, W, 0, torch)
    d = c.read(5, np.zeros(nt * 64, np.uint32)).reshape(nt, 64)[:, 56:61].astype(np.float64)
    tot = d[:, :3].sum()
    print("%s %dx%d: chunks clean %.2f%% resolved %.2f%% table %.2f%%; per tile switches to table %.1f, to fast %.1f" % (
        name, W, W, 100 * d[:, 0].sum() / tot, 100 * d[:, 1].sum() / tot, 100 * d[:, 2].sum() / tot,
        d[:, 3].mean(), d[:, 4].mean()))
c.close()
