"""The C-ABI shared library loads on a CPU-only machine and exports every symbol
include/mi_phylo.h declares (no compute without a GPU: creating an engine must fail
loudly, not fall back)."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "mi_phylo.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    from libsbn_amd import _capi
    lib = _capi.load()
    declared = _declared_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in mi_phylo.h but not exported"
    assert sorted(_capi.SYMBOLS) == declared, "ctypes table out of sync with the header"
    assert lib.mi_abi_version() == 2


def test_library_has_no_unresolved_internal_symbols():
    """ctypes binds lazily, so a launcher that was declared but never defined would only
    show up when a C++ caller links against the library: check the dynamic symbol table."""
    import subprocess
    for name in ("libmi_phylo.so", "libmi_phylo_host.so"):
        path = os.path.join(REPO, "libsbn_amd", name)
        out = subprocess.run(["nm", "-D", "-u", "-C", path], capture_output=True, text=True,
                             check=True).stdout
        internal = [line for line in out.splitlines() if "miphylo::" in line or " mih_" in line
                    or " mi_" in line]
        assert not internal, f"{name}: unresolved internal symbols: {internal}"


def test_spec_struct_layout_matches_header():
    from libsbn_amd import _capi
    assert ctypes.sizeof(_capi.EngineSpec) == 40  # ten int32 fields


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import libsbn_amd as L
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        L.Engine(L.PhyloModelSpecification(), np.zeros((3, 4), np.int32), np.ones(4))


def test_device_bytes_held_is_back_after_a_creation():
    """mi_device_bytes_held: a creation that fails (here: no device) leaves nothing held -- 0 in a
    process that never had a device --, one that succeeds holds something until the engine is
    destroyed."""
    import torch
    from libsbn_amd import _capi
    lib = _capi.load()
    before = lib.mi_device_bytes_held()
    spec = _capi.EngineSpec(3, 4, 4, 1, 0, 0, 0, 1, -1, 0)  # JC69, constant site model, no clock
    tips, weights = np.zeros((3, 4), np.int32), np.ones(4)
    handle = ctypes.c_void_p()
    rc = lib.mi_engine_create(ctypes.byref(spec), tips.ctypes.data, None, weights.ctypes.data,
                              ctypes.byref(handle))
    if torch.cuda.is_available():
        assert rc == 0, lib.mi_last_error()
        assert lib.mi_device_bytes_held() > before
        lib.mi_engine_destroy(handle)
    else:
        assert rc != 0 and b"no HIP device" in lib.mi_last_error()
        assert before == 0
    assert lib.mi_device_bytes_held() == before


def test_product_does_not_reference_the_oracle():
    """The product path must never route through oracle/ (test infrastructure)."""
    pkg = os.path.join(REPO, "libsbn_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".hpp")):
                text = open(os.path.join(root, f), errors="ignore").read()
                assert "liboracle" not in text and "oracle_lib" not in text and \
                    "phylo_oracle" not in text, f


def test_shard_range_covers_every_unit_once():
    """mi_shard_range (contiguous blocks of trees / site patterns over the shards of one
    handle, and over ranks in libsbn_amd/sharding.py): pure host arithmetic."""
    from libsbn_amd import _capi, sharding
    lib = _capi.load()
    b, c = ctypes.c_int32(), ctypes.c_int32()
    for total in (0, 1, 7, 8, 9, 100, 1000, 50000):
        for count in (1, 2, 3, 8, 16):
            seen = 0
            for s in range(count):
                assert lib.mi_shard_range(total, count, s, ctypes.byref(b), ctypes.byref(c)) == 0
                assert b.value == seen and 0 <= c.value <= total // count + 1
                assert (b.value, b.value + c.value) == sharding.tree_shard(total, s, count)
                seen += c.value
            assert seen == total
    assert lib.mi_shard_range(10, 0, 0, ctypes.byref(b), ctypes.byref(c)) != 0
    assert lib.mi_device_count() >= 0


def test_cpp_callers_build_against_the_library(tmp_path):
    """The two C++ programs that call the engine through the adapter (the reference's doctests,
    tests/cpp/engine_example.cpp, and bench.py's adapter leg, tools/engine_bench.cpp) must
    compile and link against the in-tree libraries -- on the GPU box they are built by the
    tests / by bench.py at run time, where a drift of the header would only show up then."""
    import subprocess
    lib = os.path.join(REPO, "libsbn_amd")
    for src in ("tests/cpp/engine_example.cpp", "tools/engine_bench.cpp"):
        exe = tmp_path / os.path.basename(src).replace(".cpp", "")
        subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, src), "-L" + lib,
                        "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)],
                       check=True)
        assert exe.exists()
