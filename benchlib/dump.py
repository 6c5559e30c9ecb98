"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as `DIR/<name>.npy`, so that two builds
can be compared output for output on identical inputs."""
import os

import numpy as np

MAX_BYTES = 64 << 20        # all files of one rank together


def dump_outputs(out_dir, arrays, rank=0, world=1):
    """Write each tensor of `arrays` ({name: tensor}) as float32 (float64 stays float64).  When the whole set exceeds
    MAX_BYTES, every array is cut to its share by a fixed, seeded sample of flat positions (ascending, the same on every
    run), stored as a 1-d array.  With more than one rank each rank writes its own files (`<name>.rank<r>.npy`)."""
    os.makedirs(out_dir, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        host[name] = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
    total = sum(a.nbytes for a in host.values())
    written = {}
    for name, a in host.items():
        if total > MAX_BYTES:
            keep = max(1, int(MAX_BYTES * a.nbytes / total) // a.itemsize)
            if keep < a.size:
                idx = np.sort(np.random.default_rng(20240601).choice(a.size, keep, replace=False))
                a = a.reshape(-1)[idx]
        fname = name + (".rank%d" % rank if world > 1 else "") + ".npy"
        np.save(os.path.join(out_dir, fname), a)
        written[name] = list(a.shape)
    return written
