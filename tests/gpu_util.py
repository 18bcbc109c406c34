import contextlib
import os

import numpy as np
import pytest


def need_gpu():
    from lattisense_amd._native import lib
    lib()  # fails loudly if the HIP library is not built


def rand_ct(rng, mods, polys, n, batch):
    out = np.empty((batch, polys, len(mods), n), dtype=np.uint64)
    for i, q in enumerate(mods):
        out[:, :, i, :] = rng.integers(0, q, size=(batch, polys, n), dtype=np.uint64)
    return out


@contextlib.contextmanager
def env(**switches):
    """run-time switches of the library for the block: value None = unset; the previous environment comes back after it.
    (Only switches the library reads per call, or when the block makes its own context / plan / task, see a change:
    INTEGRATION.md section 6.)"""
    old = {k: os.environ.get(k) for k in switches}
    try:
        for k, v in switches.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
