#!/usr/bin/env python
"""tools/svc_bench.py [--out profiles/svc_bench.json] [--sizes 2000,30000,100000]: SVC prediction on
the device (csrc/svm.hip through TraditionalClassifier('svm')) against SVC.predict of the same
fitted model in the same process (libsvm, one CPU thread -- the baseline, not the kernel under test).

Data: 10 Gaussian classes in 15 dimensions (the feature vector's shape), N rows split 80 / 20;
SVC(C=1.0, kernel='rbf', random_state=42).fit on the 80 % (libsvm on the CPU in both columns).
Timed, with a device sync around each region, for test-set and train-set queries:
  device_cold_s   clf.predict with nothing uploaded yet: model upload, query upload, the three
                  launches, the read-back and the libsvm redo of uncertified rows
  device_warm_s   the same call again (the model stays on the device)
  query_s         SvcIndex.query alone on queries already on the device (best of 3): pairs_per_s =
                  Nq * nSV / query_s, and fp64_fraction = pairs_per_s * OPS_PER_PAIR / FP64_VECTOR_PEAK
  sklearn_s       clf.model.predict
and the labels are compared.  Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-audioreclabs_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

D, C = 15, 10
OPS_PER_PAIR = 100.0          # estimate: ~30 for the distance, one exp (~60), C FMAs
FP64_VECTOR_PEAK = 78.6e12    # MI355X data sheet, vector FP64 FLOP/s (not measured here)


def data(N):
    rng = np.random.default_rng(N)
    y = rng.integers(0, C, N)
    X = rng.normal(0.0, 0.78, (C, D))[y] + rng.normal(size=(N, D))
    cut = N * 8 // 10
    return X[:cut], y[:cut], X[cut:], y[cut:]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench_queries(clf, Q, name):
    from src.pipeline import SvcIndex
    clf._index = None
    cold, y_dev = timed(lambda: clf.predict(Q))
    unc = clf.last_predict_stats['uncertified']
    warm, y_dev2 = timed(lambda: clf.predict(Q))
    idx, qd = SvcIndex(clf.model), torch.as_tensor(Q).to("cuda:0")
    query_s = min(timed(lambda: idx.query(qd))[0] for _ in range(3))
    sk, y_sk = timed(lambda: clf.model.predict(Q))
    pairs = float(len(Q)) * idx.nSV
    r = dict(queries=name, Nq=len(Q), device_cold_s=cold, device_warm_s=warm, query_s=query_s, sklearn_s=sk,
             speedup_cold=sk / cold, speedup_warm=sk / warm, uncertified=unc,
             labels_equal=bool(np.array_equal(y_dev, y_sk) and np.array_equal(y_dev2, y_sk)),
             pairs_per_s=pairs / query_s, fp64_fraction=pairs / query_s * OPS_PER_PAIR / FP64_VECTOR_PEAK)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "svc_bench.json"))
    ap.add_argument("--sizes", default="2000,30000,100000")
    args = ap.parse_args()
    from src.models import create_classifier
    res = dict(device=torch.cuda.get_device_name(0), shape=dict(D=D, C=C), ops_per_pair=OPS_PER_PAIR,
               fp64_vector_peak=FP64_VECTOR_PEAK, runs=[])
    Xw, yw, Qw, _ = data(1000)  # warm-up: library load, allocator
    create_classifier('svm', C=1.0, kernel='rbf').fit(Xw, yw).predict(Qw)
    for N in [int(s) for s in args.sizes.split(",")]:
        Xtr, ytr, Xte, _ = data(N)
        clf = create_classifier('svm', C=1.0, kernel='rbf')
        fit_s, _ = timed(lambda: clf.fit(Xtr, ytr))
        run = dict(N=N, fit_s=fit_s, nSV=int(clf.model.support_vectors_.shape[0]), queries=[])
        print(json.dumps(dict(N=N, fit_s=fit_s, nSV=run["nSV"])), flush=True)
        run["queries"].append(bench_queries(clf, Xte, "test"))
        run["queries"].append(bench_queries(clf, Xtr, "train"))
        res["runs"].append(run)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
