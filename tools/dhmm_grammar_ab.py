#!/usr/bin/env python
"""DSP_LIB_PATH=dsp-audioreclabs_amd/lib/libdsp_audiorec_wpb1.so tools/dhmm_grammar_ab.py: one leg of the A / B of
dsp_dhmm_decode_grammar's waves per workgroup (profiles/dhmm_grammar_ab.txt).  The libraries come
from ``make -C dsp-audioreclabs_amd/csrc grammarvariant V=wpb1 D="-DGRAMMAR_WPB=1"`` (and 2, 4); run each in its own
process, in alternating rounds.  10 000 utterances of 52 .. 181 uniform random frames, 64 models x 32 / 16 / 8 states,
K = 64, a random grammar with 30 % of pair forbidden; medians of 7 after 2 warm-ups under device events; three
utterances of each call are compared bit for bit with the numpy restatement.  Prints one line."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("dsp-audioreclabs_amd", "tests", "tools"):
    sys.path.insert(0, os.path.join(REPO, d))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dhmm_bench as DB  # noqa: E402
import dhmm_grammar_bench as GB  # noqa: E402
import dtw_bench as D  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("dhmm_grammar_ab needs the MI355X: nothing is measured without it")
    import dhmm_grammar_reference as GR
    import dhmm_reference as DR
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2)
    N, K = 10000, 64
    n = rng.integers(52, 182, N).astype(np.int32)
    sym_host = rng.integers(0, K, (N, 181)).astype(np.int32)
    sym, lens = torch.as_tensor(sym_host, device=dev), torch.as_tensor(n, device=dev)
    enter, pair, leave = GR.random_grammar(64, seed=4, forbid=0.3)
    out = [os.path.basename(os.environ.get("DSP_LIB_PATH", "libdsp_audiorec.so"))]
    for S in (32, 16, 8):
        big = DB.random_model_set(64, S, K, seed=3)
        outs, ms = D.timed(GB.grammar_call(big, sym, lens, enter, pair, leave, 16, dev), 7)
        want = GR.decode(DR.Model(big.emit, big.stay, big.adv, big.n_states), sym_host[:3], n[:3], enter, pair, leave, 16)
        out.append("S=%d %.3f ms %s" % (S, float(np.median(ms)), GB.bits_equal([o.cpu().numpy()[:3] for o in outs], want)))
    print("  ".join(out), flush=True)


if __name__ == "__main__":
    main()
