"""Writes mlp_parity_inputs.npz: the SHA-256 of every array tests/mlp_reference.parity_inputs
returns for the four parity shapes, and the first four values of each.  The committed file was
written before parity_inputs took its seeds from an explicit table, so it pins the inputs those
cases have always had; run this again only to pin a new name, never to refresh an old one.

    python tests/golden/make_mlp_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import mlp_reference as R  # noqa: E402

NAMES = ('config_108', 'n_below_batch', 'odd_16', 'tiny_4')
FIELDS = ('X', 'y', 'perm', 'packed0')


def digests(name):
    out = {}
    arrays = dict(zip(FIELDS, R.parity_inputs(name)[5:]))
    for field, a in arrays.items():
        a = np.ascontiguousarray(a)
        out["%s/%s/sha256" % (name, field)] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
        out["%s/%s/head" % (name, field)] = a.reshape(-1)[:4].copy()
        out["%s/%s/shape" % (name, field)] = np.array(a.shape, dtype=np.int64)
    return out


if __name__ == "__main__":
    pins = {}
    for n in NAMES:
        pins.update(digests(n))
    np.savez(os.path.join(HERE, "mlp_parity_inputs.npz"), **pins)
