"""Generator of ``griffinlim.npz`` (BUILD CONTAINER ONLY; never imported by a test).

Imports the reference's ``dataloaders/stft.py`` and records what its ``STFT.inverse`` and ``griffin_lim`` compute.  The
file's third-party imports that are absent here get in-process stand-ins: ``librosa.util.{pad_center, normalize, tiny}``
(their published definitions for the arguments ``stft.py`` passes) and the ``Variable`` name ``inverse`` uses without
importing it (`stft.py:171`).  Only arrays are written: magnitudes, initial angles and the two results per case.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden._refimport import REF      # noqa: E402 -- where the reference checkout lies (DWS_REFERENCE)
CASES = {"n64": (64, 16, 12), "n1024": (1024, 256, 6)}          # name -> (filter_length, hop_length, frames)


def _stub_librosa():
    def pad_center(data, size=None, axis=-1, **kw):
        n = data.shape[axis]
        lpad = (size - n) // 2
        widths = [(0, 0)] * data.ndim
        widths[axis] = (lpad, size - n - lpad)
        return np.pad(data, widths, **kw)

    def normalize(S, norm=np.inf, **kw):
        assert norm is None            # what `stft.py:57` passes: the identity
        return S

    def tiny(x):
        x = np.asarray(x)
        dtype = x.dtype if np.issubdtype(x.dtype, np.floating) else np.dtype(np.float32)
        return np.finfo(dtype).tiny

    lib = types.ModuleType("librosa")
    lib.util = types.ModuleType("librosa.util")
    lib.util.pad_center, lib.util.normalize, lib.util.tiny = pad_center, normalize, tiny
    sys.modules["librosa"], sys.modules["librosa.util"] = lib, lib.util


def load_reference_stft():
    if not os.path.isdir(REF):
        raise RuntimeError(f"reference checkout not found at {REF}")
    _stub_librosa()
    spec = importlib.util.spec_from_file_location("reference_stft", os.path.join(REF, "dataloaders", "stft.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.Variable = torch.autograd.Variable
    return mod


def main():
    ref = load_reference_stft()
    from tests import griffinlim_reference as glr
    out = {}
    for name, (n_fft, hop, frames) in CASES.items():
        fn = ref.STFT(filter_length=n_fft, hop_length=hop, win_length=n_fft)
        x = torch.from_numpy(glr.test_signal(2, (frames - 1) * hop).astype(np.float32))
        with torch.no_grad():
            mag, _ = fn.transform(x)
            np.random.seed(20240 + n_fft)
            state = np.random.get_state()
            angles = np.angle(np.exp(2j * np.pi * np.random.rand(*mag.size()))).astype(np.float32)     # `stft.py:74-75`
            inv = fn.inverse(mag, torch.from_numpy(angles)).squeeze(1)
            np.random.set_state(state)              # griffin_lim draws the same angles
            gl = ref.griffin_lim(mag, fn, n_iters=4)
        assert mag.shape == (2, n_fft // 2 + 1, frames) and inv.shape == (2, (frames - 1) * hop) == gl.shape
        out[name + "_magnitude"] = mag.numpy()
        out[name + "_angles"] = angles
        out[name + "_inverse"] = inv.numpy()
        out[name + "_griffin_lim4"] = gl.numpy()
    path = os.path.join(HERE, "griffinlim.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
