"""What every library of build.LIBS owes: it is built from the tree's sources and says so, it
exports exactly what its header declares and its module lists, and nothing that belongs to another
library; and `_loader.load`, the one way they are loaded, refuses a missing or stale file. CPU only."""

import os
import re
import subprocess

import pytest

from nmmo_amd import _loader, _native, build, heads, lstm, ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# library of build.LIBS: (module, symbol prefix, header, symbol names pinned here as literals,
# whether the header declares exactly those, each once, or at least those)
TABLE = {
    "hip": (_native, "nmmo", "nmmo_hip.h", set(), False),
    "heads": (heads, "nmh", "nmmo_heads.h", {"nmh_forward", "nmh_backward", "nmh_last_error"}, False),
    "ppo": (ppo, "nmp", "nmmo_ppo.h", {"nmp_loss", "nmp_last_error", "nmp_build_info"}, True),
    "lstm": (lstm, "nml", "nmmo_lstm.h",
             {"nml_cell", "nml_seq_forward", "nml_seq_backward", "nml_last_error", "nml_build_info"}, True),
}
NAMES = sorted(build.LIBS)  # a library without a row above fails every test below


def exports(name):
    """The defined dynamic text symbols of library `name` that start with "nm"."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.lib_path(name)]).decode()
    return {s for s in re.findall(r"\sT\s(\w+)", out) if s.startswith("nm")}


def header_text(name):
    return open(os.path.join(ROOT, "include", TABLE[name][2])).read()


@pytest.mark.parametrize("name", NAMES)
def test_library_is_built_from_the_tree_and_loads(name):
    m, prefix = TABLE[name][:2]
    assert not build.stale(name)
    info = getattr(m.lib(), prefix + "_build_info")().decode()
    assert "src=" + build.source_hash(name) in info and "arch=gfx950" in info and "fp_contract=off" in info


@pytest.mark.parametrize("name", NAMES)
def test_exports_equal_header_declarations_and_module_symbols(name):
    m, prefix, _, pinned, exact = TABLE[name]
    assert exports(name) == set(m.SYMBOLS)
    for sym in m.SYMBOLS:
        getattr(m.lib(), sym)
    if name == "hip":  # tests/test_abi.py compares libnmmo_hip.so with its header
        return
    decl = re.findall(rf"{prefix.upper()}_API\s+[\w\s\*]+?\b({prefix}_\w+)\s*\(", header_text(name))
    assert pinned <= set(decl)
    if exact:
        assert set(decl) == pinned and len(decl) == len(pinned)
    assert set(decl) == exports(name)
    assert set(decl) == set(m.SYMBOLS)


@pytest.mark.parametrize("name", NAMES)
def test_no_library_or_header_carries_another_librarys_prefix(name):
    # the headers name one another's files (nmmo_hip.h, libnmmo_ppo.so) in their comments: those
    # are not symbols
    syms, text = exports(name), re.sub(r"\b(?:lib)?nmmo_\w+\.(?:h|so)\b", "", header_text(name))
    for other in NAMES:
        theirs = TABLE[other][1] + "_"
        if other != name:
            assert not {s for s in syms if s.startswith(theirs)}, other
            assert theirs not in text, other


# _loader.load itself, on libnmmo_heads.so: called directly, because a module's lib() is memoised
OTHER = "0123456789abcdef"


def load_heads(path=build.lib_path("heads")):
    return _loader.load("heads", path, heads.HeadsError, "nmh", heads.declare, "no fallback for this one")


def test_loader_refuses_a_missing_library(tmp_path):
    path = str(tmp_path / "libnmmo_heads.so")
    with pytest.raises(heads.HeadsError) as e:
        load_heads(path)
    assert path in str(e.value) and "is missing" in str(e.value) and "(no fallback for this one)" in str(e.value)


def test_loader_refuses_a_library_built_from_other_sources(monkeypatch):
    have = build.source_hash("heads")
    monkeypatch.delenv("NMMO_ALLOW_STALE", raising=False)
    monkeypatch.setattr(build, "source_hash", lambda name="hip": OTHER)
    with pytest.raises(heads.HeadsError) as e:
        load_heads()
    msg = str(e.value)
    assert build.lib_path("heads") in msg and "was built from other sources" in msg
    assert f"src={have}" in msg and f"tree={OTHER}" in msg


def test_loader_allows_a_stale_library_on_request(monkeypatch):
    monkeypatch.setenv("NMMO_ALLOW_STALE", "1")
    monkeypatch.setattr(build, "source_hash", lambda name="hip": OTHER)
    L = load_heads()
    assert L.nmh_forward.argtypes and _loader.build_info(L, "nmh")["arch"] == "gfx950"
