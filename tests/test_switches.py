"""The MI_PHYLO_* environment switches: read in one place of the library when an engine is
created, listed once in README's table, and refused -- before any device work -- when a value is
outside a switch's accepted set."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "libsbn_amd", "csrc")
# the Python loader's own variables (libsbn_amd/_capi.py), listed apart from the table
LOADER = {"MI_PHYLO_LIBRARY", "MI_PHYLO_NO_TORCH_PRELOAD"}
SOURCES = (".h", ".hpp", ".hip", ".cpp")


def _names(text):
    return set(re.findall(r"\bMI_PHYLO_[A-Z0-9_]*[A-Z0-9]", text))


def _read(path):
    with open(path, errors="ignore") as f:
        return f.read()


def _getenv_files():
    found = []
    for root, dirs, files in os.walk(CSRC):
        dirs[:] = [d for d in dirs if not d.startswith("build")]
        for f in files:
            if f.endswith(SOURCES) and "getenv" in _read(os.path.join(root, f)):
                found.append(os.path.relpath(os.path.join(root, f), CSRC))
    return found


def _readme_table():
    rows = [line for line in _read(os.path.join(REPO, "README.md")).splitlines()
            if line.startswith("| `MI_PHYLO_")]
    return {re.match(r"\| `(MI_PHYLO_[A-Z0-9_]+)`", line).group(1) for line in rows}


def test_one_file_reads_the_environment():
    files = _getenv_files()
    assert len(files) == 1, files


def test_readme_table_lists_exactly_the_parsed_switches():
    (parser,) = _getenv_files()
    parsed = _names(_read(os.path.join(CSRC, parser)))
    table = _readme_table()
    assert parsed == table, (sorted(parsed - table), sorted(table - parsed))
    assert not LOADER & table
    readme = _read(os.path.join(REPO, "README.md"))
    for name in LOADER:
        assert name in readme


def test_every_switch_the_tests_and_tools_name_is_in_the_table():
    known = _readme_table() | LOADER
    paths = [os.path.join(REPO, "bench.py")]
    for top in ("tests", "tools"):
        for root, dirs, files in os.walk(os.path.join(REPO, top)):
            dirs[:] = [d for d in dirs if d not in ("golden", "__pycache__")]
            paths += [os.path.join(root, f) for f in files]
    unknown = {}
    for path in paths:
        extra = _names(_read(path)) - known
        if extra:
            unknown[os.path.relpath(path, REPO)] = sorted(extra)
    assert not unknown, unknown


def _create(kind):
    import libsbn_amd as L
    rng = np.random.default_rng(5)
    if kind == "20-state":
        tips = rng.integers(0, 20, size=(4, 7)).astype(np.int32)
        model = (np.ones(190), np.full(20, 0.05))
        return L.Engine(L.PhyloModelSpecification("WAG", "weibull+4", "strict"), tips, np.ones(7),
                        reversible_model=model)
    tips = rng.integers(0, 4, size=(4, 7)).astype(np.int32)
    kw = {"shard_devices": [0]} if kind == "sharded" else {}
    return L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, np.ones(7), **kw)


KINDS = ("4-state", "20-state", "sharded")
BAD = (("MI_PHYLO_GRADIENT_WALK", "v1"), ("MI_PHYLO_FUSED_FENCE", "agnet"), ("MI_PHYLO_AA_RING", "3"),
       ("MI_PHYLO_WALK_TILE_REGS", "5"), ("MI_PHYLO_PLV_BYTES", "12x"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,value", BAD)
def test_creation_refuses_an_unknown_value(monkeypatch, kind, name, value):
    monkeypatch.setenv(name, value)
    with pytest.raises(RuntimeError, match=f"^{name}={re.escape(value)}: expected "):
        _create(kind)


def test_refusal_names_the_accepted_values(monkeypatch):
    monkeypatch.setenv("MI_PHYLO_GRADIENT_WALK", "v1")
    with pytest.raises(RuntimeError) as err:
        _create("4-state")
    assert str(err.value) == "MI_PHYLO_GRADIENT_WALK=v1: expected v2|v3"


@pytest.mark.parametrize("kind", KINDS)
def test_valid_switches_reach_the_device_check(monkeypatch, kind):
    """Accepted values pass the parser: a machine without a GPU then gets the engine's own
    "no HIP device" error, a machine with one an engine."""
    from libsbn_amd import _capi
    for name, value in (("MI_PHYLO_GRADIENT_WALK", "v2"), ("MI_PHYLO_FUSED_FENCE", "agent"),
                        ("MI_PHYLO_AA_RING", "4"), ("MI_PHYLO_WALK_TILE_REGS", "3"),
                        ("MI_PHYLO_PLV_BYTES", "3000000"), ("MI_PHYLO_FUSED_SPIN_MS", "20"),
                        ("MI_PHYLO_MACRO_SLOTS", "seq"), ("MI_PHYLO_TIP_TILES", "0")):
        monkeypatch.setenv(name, value)
    if _capi.load().mi_device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            _create(kind)
    else:
        _create(kind).close()
