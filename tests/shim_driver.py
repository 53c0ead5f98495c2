"""The test drivers of stereo-dso-g2o_amd/host (one C++ program per shim test module): build one, hand it a problem as raw arrays
(<dir>/<name>.bin, see host/driver_io.h), run it, read what it printed and dumped (<dir>/out_<name>.bin)."""
import os
import subprocess

import numpy as np

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stereo-dso-g2o_amd", "host")


def exe(name):
    return os.path.join(HOST, name)


def _make(*args):
    r = subprocess.run(["make", "-C", HOST] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def build(name):
    """the program, brought up to date"""
    _make("-s", name)
    return exe(name)


def rebuild(name):
    """CPU: the shim + the driver compile from scratch against the ABI header with the plain host compiler"""
    _make("-B", name)
    assert os.path.exists(exe(name))


class Run:
    def __init__(self, d, stdout):
        self.d, self.stdout, self.lines = str(d), stdout, stdout.strip().splitlines()

    def out(self, name, dtype):
        return np.fromfile(os.path.join(self.d, "out_" + name + ".bin"), dtype=dtype)


def run(name, d, arrays, *args, mode=None, timeout=300):
    """write `arrays` into d, run `name [mode] d args...`"""
    for k, a in arrays.items():
        np.ascontiguousarray(a).tofile(os.path.join(str(d), k + ".bin"))
    r = subprocess.run([exe(name)] + ([mode] if mode else []) + [str(d)] + list(args), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return Run(d, r.stdout)


# ---- the immature-point record of the drivers (host/driver_io.h: point_from_record / dump_points): 30 floats and a status byte per point
_SCALARS = (("u", 0), ("v", 1), ("my_type", 2), ("idepth_min", 3), ("idepth_max", 4), ("quality", 5), ("energyTH", 26), ("lastTracePixelInterval", 29))
_BLOCKS = (("color", 6, 14), ("weights", 14, 22), ("gradH", 22, 26), ("lastTraceUV", 27, 29))


def pack_points(S):
    """the members of immature_ref -> the record"""
    f = np.zeros((len(S["u"]), 30), np.float32)
    for k, c in _SCALARS:
        f[:, c] = S[k]
    for k, lo, hi in _BLOCKS:
        f[:, lo:hi] = S[k]
    return f, np.ascontiguousarray(S["lastTraceStatus"], np.uint8)


def unpack_points(f, st):
    """the record -> the members of immature_ref"""
    f = f.reshape(-1, 30)
    S = {k: f[:, c].copy() for k, c in _SCALARS}
    S.update({k: f[:, lo:hi].copy() for k, lo, hi in _BLOCKS}, lastTraceStatus=st)
    return S
