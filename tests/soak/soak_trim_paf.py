"""Randomised soak of the whole trim-paf command on generated files (tests/trim_util.py) against the oracle CLI's bytes, every configuration,
all three routes: `rb trim-paf`, trim_driver.ResidentTrim, trim_driver.overlapping_paf_recs.  `python tests/soak/soak_trim_paf.py [cases]`"""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402  (before the library: tests/conftest.py says why)
import rustybam_amd  # noqa: E402
from oracle import pyoracle as oracle  # noqa: E402
from rustybam_amd import trim_driver  # noqa: E402
from rbtest_util import recs_from_lines  # noqa: E402
from trim_util import CONFIGS, format_recs, format_resident, oracle_args, parse, random_trim_paf, rb_args  # noqa: E402

RB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "rustybam_amd", "rb")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device("cuda", 0)
torch.cuda.set_stream(torch.cuda.Stream(dev))
eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
for case in range(n):
    seed = 9000 + case
    text = random_trim_paf(seed, 60 + 20 * (case % 5))
    r = recs_from_lines(text.decode().splitlines())
    rank = {q: i for i, q in enumerate(sorted(set(r.q_name)))}
    group = np.array([rank[q] for q in r.q_name])
    for cfg, c in CONFIGS.items():
        rc, want = oracle.cli(*oracle_args(cfg), stdin=text)
        assert rc == 0, (seed, cfg)
        p = subprocess.run([RB, *rb_args(cfg)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0 and p.stdout == want, (seed, cfg, "rb trim-paf")
        T = trim_driver.ResidentTrim(eng, torch, dev, r.ops, r.op_off, r.t_st, r.t_en, r.q_st, r.q_en, r.strand, group)
        norm0 = T.d_norm.cpu().numpy().view(rustybam_amd.NORM_DT)[:r.n].copy()
        T.run(c["scores"], c["policy"])
        d_new, new_off, norm = T.gather()
        got = format_resident(r, norm0, norm, d_new.cpu().numpy().view(np.uint32), new_off, T.order, keep=~T.contained if c["remove"] else None)
        assert got.encode() == want, (seed, cfg, "ResidentTrim")
        del d_new
        T.release()
        out = trim_driver.overlapping_paf_recs(eng, parse(text), c["scores"], c["remove"], c["policy"])
        assert format_recs(out).encode() == want, (seed, cfg, "overlapping_paf_recs")
    print(f"case {case} (seed {seed}): {r.n} records, every configuration, three routes: the oracle's bytes", flush=True)
torch.cuda.synchronize()
eng.close()
