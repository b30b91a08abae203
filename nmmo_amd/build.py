"""Build the native libraries in-tree with hipcc for gfx950 (no JIT cache: the libraries ship with
the repo snapshot to the GPU box). `LIBS` has one row per library; a new library is a new row."""

from __future__ import annotations

import concurrent.futures
import functools
import hashlib
import os
import subprocess
import sys
import tempfile
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(HERE, "..", "include")
LIB_DIR = os.path.join(HERE, "lib")
ARCH = os.environ.get("NMMO_OFFLOAD_ARCH", "gfx950")


class Lib(NamedTuple):
    file: str  # under LIB_DIR
    sources: list  # under CSRC; each is a translation unit of its own
    headers: list  # the csrc headers that enter the source hash
    include: list  # the include/ headers that enter the source hash
    link: list = []  # extra link flags


# The product library and, each a library of its own so that libnmmo_hip.so's exports and source
# hash stay what the C-ABI tests and bench.py pin: the fused action heads (include/nmmo_heads.h),
# the fused PPO minibatch loss (include/nmmo_ppo.h), the fused LSTM recurrence (include/nmmo_lstm.h).
LIBS = {
    "hip": Lib("libnmmo_hip.so",
               ["mapgen.hip", "tick.hip", "obs.hip", "wrap.hip", "storage.hip", "wire.hip", "wire_obs.hip",
                "native_obs.hip", "flat_obs.hip", "p2p.hip", "capi.hip"],
               ["agent_obs.h", "common.h", "host_api.h", "kernels.h", "obs_layout.h", "wire.h"], ["nmmo_hip.h"],
               ["-ldl"]),
    "heads": Lib("libnmmo_heads.so", ["heads.hip", "tile_enc.hip", "item_enc.hip", "player_enc.hip", "embed_enc.hip",
                  "decoder.hip"],
                 ["common.h", "host_api.h", "heads_dev.h", "heads_host.h", "item_dev.h", "player_dev.h", "set_dev.h"],
                 ["nmmo_hip.h", "nmmo_heads.h"]),
    "ppo": Lib("libnmmo_ppo.so", ["ppo.hip"], ["host_api.h"], ["nmmo_ppo.h"]),
    "lstm": Lib("libnmmo_lstm.so", ["lstm.hip"], ["host_api.h"], ["nmmo_lstm.h"]),
}
SOURCES, HEADERS = LIBS["hip"].sources, LIBS["hip"].headers
LIB_PATH = os.path.join(LIB_DIR, LIBS["hip"].file)
STAMPS_PATH = os.path.join(LIB_DIR, "libnmmo_hip_stamps.so")
# the product library's sources with -DNMMO_TEST_HOOKS: the same kernels plus read-only test hooks
# (capi.hip nmmo_debug_obs_row_state), loaded through NMMO_LIB by the tests that need them
HOOKS_PATH = os.path.join(LIB_DIR, "libnmmo_hip_hooks.so")
FLAGS = [
    f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Werror",
    # no FMA contraction: hipcc contracts even __dadd_rn(__dmul_rn(..)) pairs, and the float /
    # double reward, wrapper and advantage arithmetic must round op by op like the oracle
    "-ffp-contract=off",
]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.sep not in cand or os.path.exists(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def lib_path(name: str = "hip") -> str:
    return os.path.join(LIB_DIR, LIBS[name].file)


def source_hash(name: str = "hip") -> str:
    """sha256 (first 16 hex) over the HIP sources and headers library `name` is compiled from; the
    library embeds it (<prefix>_build_info) and _loader.load() refuses a library built from other
    sources, so a run always reflects the tree it ships with."""
    row = LIBS[name]
    h = hashlib.sha256()
    for f in [os.path.join(CSRC, f) for f in row.sources + row.headers] + [
            os.path.join(INCLUDE, f) for f in row.include]:
        with open(f, "rb") as fh:
            h.update(os.path.basename(f).encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def stale(name: str = "hip") -> bool:
    """True unless library `name` exists and embeds its current source hash."""
    if not os.path.exists(lib_path(name)):
        return True
    with open(lib_path(name), "rb") as fh:
        return ("src=" + source_hash(name)).encode() not in fh.read()


def _embeds(path: str, name: str) -> bool:
    if not os.path.exists(path):
        return False
    with open(path, "rb") as fh:
        return ("src=" + source_hash(name)).encode() in fh.read()


def build_lib(name: str, force: bool = False, verbose: bool = False, stamps: bool = False, hooks: bool = False) -> str:
    """Library `name`; `stamps=True` builds the product library's diagnostic variant (phase clock
    stamps, tools/stamps.py) to lib/libnmmo_hip_stamps.so instead, `hooks=True` its test-hook
    variant to lib/libnmmo_hip_hooks.so (rebuilt when it does not embed the current source hash)."""
    row = LIBS[name]
    if (stamps or hooks) and name != "hip":
        raise ValueError("only the product library has variants")
    out = STAMPS_PATH if stamps else HOOKS_PATH if hooks else lib_path(name)
    if not force and hooks and _embeds(out, name):
        return out
    if not force and not stamps and not hooks and not stale(name):
        return out
    os.makedirs(LIB_DIR, exist_ok=True)
    tmp = out + ".tmp"
    flags = [*FLAGS, *(["-DNMMO_STAMPS"] if stamps else []), *(["-DNMMO_TEST_HOOKS"] if hooks else []), f'-DNMMO_SRC_HASH="{source_hash(name)}"']
    # one hipcc per source in parallel (every kernel lives in its own translation unit), then link
    with tempfile.TemporaryDirectory(prefix="nmmo_build_") as d:
        objs = [os.path.join(d, f + ".o") for f in row.sources]
        cmds = [[_hipcc(), *flags, "-c", os.path.join(CSRC, f), "-o", o] for f, o in zip(row.sources, objs)]
        if verbose:
            print("\n".join(" ".join(c) for c in cmds), file=sys.stderr)
        jobs = max(1, min(len(cmds), os.cpu_count() or 1, int(os.environ.get("MAX_JOBS", "8"))))
        with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
            for f in [ex.submit(subprocess.check_call, c) for c in cmds]:
                f.result()
        subprocess.check_call([_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", *objs, *row.link, "-o", tmp])
    os.replace(tmp, out)
    return out


build = functools.partial(build_lib, "hip")
build_hooks = functools.partial(build_lib, "hip", hooks=True)
build_heads = functools.partial(build_lib, "heads")
build_ppo = functools.partial(build_lib, "ppo")
build_lstm = functools.partial(build_lib, "lstm")


if __name__ == "__main__":
    for lib_name in LIBS:
        print(build_lib(lib_name, force="--force" in sys.argv, verbose=True))
    print(build_hooks(force="--force" in sys.argv, verbose=True))
