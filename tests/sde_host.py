"""What the host tests of the gSDE heads share (tests/test_sde_math.py, test_sde_squash_math.py,
test_sde_eval_math.py): the stand-alone replay programs of gym-usv_amd/csrc/usv_sde_math.hpp, built plain and with
host sanitizers, how they are run, and the library's usv_sde struct."""
import ctypes
import platform
import subprocess

import numpy as np


def compile_replay(d, main, variants=("plain", "san")):
    """The replay program ``main`` in directory ``d``, plain (-O3 for a target with FMA, where the compiler would
    contract) and with AddressSanitizer + UBSan (both stand-alone host binaries): {"plain": exe, "san": exe}, or
    those of ``variants``."""
    from gym_usv_amd.build import CSRC, hipcc
    src = d / "replay.cpp"
    src.write_text(main)
    fma = ["-mfma"] if platform.machine() in ("x86_64", "AMD64") else []
    out = {}
    flags_of = {"plain": ["-O3", *fma],
                "san": ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]}
    for name in variants:
        flags = flags_of[name]
        exe = d / f"replay_{name}"
        subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", *flags, f"-I{CSRC}", "-o", str(exe), str(src)],
                       check=True)
        out[name] = str(exe)
    return out


def run_replay(exe, argv, arrays, fields):
    """Runs ``exe argv`` with the float32 ``arrays`` on stdin; stdout parsed as ``fields`` ((name, dtype, shape) in
    order, nothing left over).  Returns the arrays by name and the integers after "C " on stderr."""
    data = b"".join(np.ascontiguousarray(x, np.float32).tobytes() for x in arrays)
    p = subprocess.run([exe, *(str(a) for a in argv)], input=data, capture_output=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    o, at, out = p.stdout, 0, {}
    for name, dt, shape in fields:
        cnt = int(np.prod(shape))
        out[name] = np.frombuffer(o, dt, cnt, at).reshape(shape)
        at += 4 * cnt
    assert at == len(o)
    return out, [int(x) for x in p.stderr.decode().split("C ", 1)[1].split()]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load_lib():
    """The library, built if stale."""
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def make_sde(**kw):
    from gym_usv_amd import _lib
    f = dict(n=4, latent_dim=8, act_dim=2, reserved=0, seed=1, gid0=0)
    low, high = kw.pop("low", (0.0, -1.0, 0.0, 0.0)), kw.pop("high", (1.0, 1.0, 0.0, 0.0))
    f.update(kw)
    return _lib.UsvSde(low=(ctypes.c_float * 4)(*low), high=(ctypes.c_float * 4)(*high), **f)
