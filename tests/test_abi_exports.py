"""CPU-side checks of the boundary: the library builds for gfx950, loads without a GPU and exports
every symbol include/phdhip.h declares; the ctypes parameter block matches the C struct."""
import ctypes as C
import os
import re
import struct
import subprocess
import tempfile

from monorfs_amd import _lib
from monorfs_amd.abi import PhdParams, prm3d_defaults

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "phdhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(phd_[a-z_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported():
    so = _lib.build()
    lib = C.CDLL(so)
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "libphdhip.so does not export %s" % n
    assert set(names) == set(_lib.EXPORTS)


def test_params_struct_matches_c_defaults():
    lib = _lib.load()
    assert lib.phd_api_version() == 4
    c = PhdParams()
    lib.phd_default_params(C.byref(c), 7, 640, 33)
    py = prm3d_defaults(7, 640, 33)
    for name, _ in PhdParams._fields_:
        a, b = getattr(c, name), getattr(py, name)
        if hasattr(a, "__len__"):
            assert list(a) == list(b), name
        else:
            assert a == b, name


def test_create_fails_loudly_without_device_or_bad_params():
    import torch
    lib = _lib.load()
    p = prm3d_defaults(4, 600, 16)
    p.max_components = 10   # < max_quantity
    assert not lib.phd_create(C.byref(p), 0)
    assert b"capacities" in lib.phd_create_error()
    # MaxQuantity beyond what one particle's prune can keep in LDS is refused at creation, not at the first launch
    p = prm3d_defaults(4, 6000, 16)
    p.max_quantity = 6000
    assert not lib.phd_create(C.byref(p), 0)
    assert b"max_quantity too large" in lib.phd_create_error()
    if not torch.cuda.is_available():
        p = prm3d_defaults(4, 600, 16)
        assert not lib.phd_create(C.byref(p), 0)
        assert b"no HIP device" in lib.phd_create_error() or b"device" in lib.phd_create_error()


def prune_lds_bytes(cutcap, nb=2048):
    """prune_lds(cutcap).bytes of monorfs_amd/csrc/phd_prune.h, restated (PRUNE_NB = 2048): the library states the figure only
    where it refuses a MaxQuantity, which is where test_prune_lds_at_1024 holds this restatement against it"""
    cc = (cutcap + 1) & ~1
    ns = 512
    while ns < 2 * cutcap:
        ns <<= 1
    x = (cc // 2 + 1) & ~1
    rest = 2 * cc + 2 * cc + cc // 2 + (nb + 2) // 4 + 1 + 64 + 2 * (cc // 4 + 1) + 4    # (64: the absorbed flags, 64 bits per lane)
    ranked = ns + 516 + (ns * 2) // 3 + 2
    need = max(ns, rest, ranked)
    return (x + need + 136) * 8, rest, ranked


def static_lds_of(so, wanted):
    """{kernel: static LDS bytes} of the gfx950 kernels whose names contain one of `wanted`, from the code object's metadata"""
    blob = open(so, "rb").read()
    at = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert at >= 0, "no offload bundle in %s" % so
    count, = struct.unpack_from("<Q", blob, at + 24)
    pos, image = at + 32, None
    for _ in range(count):
        off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
        triple = blob[pos + 24:pos + 24 + tlen]
        pos += 24 + tlen
        if b"gfx950" in triple:
            image = blob[at + off:at + off + size]
    assert image, "no gfx950 code object in %s" % so
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(image)
        f.flush()
        readelf = os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "llvm", "bin", "llvm-readelf")
        notes = subprocess.check_output([readelf, "--notes", f.name]).decode()
    found = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+)(?:(?!\.group_segment_fixed_size).)*?\.name:\s*(\S+)", notes, re.S):
        if any(k in m.group(2) for k in wanted):
            found[m.group(2)] = int(m.group(1))
    return found


def test_prune_lds_at_1024():
    """The prune's working set decides how many workgroups a CU holds: at MaxQuantity 600 it is the ranked ordering's arrays
    (which the merge half's lists must stay inside), at 1024 the lists themselves — the absorbed flags among them, 64 bits per
    lane so that they reach every row phd_create admits —, and three workgroups of k_prune_merge or k_emit_prune must still
    fit a CU's 160 KB there, static LDS included."""
    lib = _lib.load()
    for q in (3600, 4000, 4098, 5000, 6000, 9000):      # (both sort widths that occur up there, an odd half)
        p = prm3d_defaults(1, q, 8)
        p.max_quantity = q
        assert not lib.phd_create(C.byref(p), 0)
        m = re.search(rb"needs (\d+) bytes", lib.phd_create_error())
        assert m and int(m.group(1)) == prune_lds_bytes(q)[0], (q, lib.phd_create_error(), prune_lds_bytes(q))
    bytes600, rest600, ranked600 = prune_lds_bytes(600)
    assert rest600 <= ranked600, "the merge half's lists outgrow the ranked ordering's arrays at MaxQuantity 600: %d > %d doubles" % (rest600, ranked600)
    bytes1024, rest1024, ranked1024 = prune_lds_bytes(1024)
    assert rest1024 > ranked1024
    static = static_lds_of(_lib.build(), ("k_prune_merge", "k_emit_prune"))
    assert len(static) == 3, static        # k_prune_merge, k_emit_prune with and without a depth map
    for kernel, fixed in static.items():
        assert 3 * (bytes1024 + fixed) <= 160 * 1024, "%s: three workgroups need 3 x (%d + %d) bytes of LDS" % (kernel, bytes1024, fixed)


def test_product_does_not_reference_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "monorfs_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp", ".hpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "libphd_oracle" not in text and "import orc" not in text, f
