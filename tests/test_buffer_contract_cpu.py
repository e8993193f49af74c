"""The buffer validator of the Python device wrappers (s3client_amd/hashing.py _device_buffer)
against duck-typed stand-ins: one case per rejection reason per kind of argument, the accepting
cases, and a check of hashing.py's source that no wrapper reads a tensor's data_ptr() by itself.
No device and no torch."""
import ast
import ctypes
import inspect

import pytest

from s3client_amd import hashing
from tests.launch_contract import FakeTensor

check = hashing._device_buffer

# (argument, bytes needed, alignment include/s3hash.h states) for every kind of device argument
KINDS = [("data", 1000, 1),
         ("digests", 32 * 16, 16),          # SHA-256 / MD5 digests
         ("digests", 20 * 16, 4),           # SHA-1 digests
         ("crcs", 4 * 16, 4), ("crcs", 8 * 16, 8),
         ("expected", 32 * 16, 4), ("mask", 16, 1),
         ("seeds", 32 * 16, 16), ("out", 32 * 40, 16), ("chunk_digests", 32 * 24, 16),
         ("signatures", 32 * 40, 16), ("checksums", 4 * 16, 4), ("checksums", 8 * 16, 8),
         ("trailer_out", 32 * 16, 16), ("clock buffer", 0, 8)]
IDS = [f"{n}-{a}" for n, _, a in KINDS]
BASE = 0x7F0000001000  # 4 KiB aligned


@pytest.mark.parametrize("name, need, align", KINDS, ids=IDS)
def test_accepts_exact_size(name, need, align):
    """Exactly the bytes needed, at an aligned address: the pointer comes back unchanged."""
    p = check(name, FakeTensor(need, BASE), need, 0, align)
    assert isinstance(p, ctypes.c_void_p) and (p.value or 0) == (BASE if need else 0)


@pytest.mark.parametrize("name, need, align", KINDS, ids=IDS)
def test_rejects_host_tensor(name, need, align):
    with pytest.raises(ValueError, match=f"{name} must be a device tensor"):
        check(name, FakeTensor(need + 64, BASE, cuda=False), need, 0, align)


def test_rejects_what_is_not_a_tensor():
    import numpy as np
    for t in (np.zeros(64, np.uint8), b"x" * 64, None, 1234):
        with pytest.raises(ValueError, match="data must be a device tensor"):
            check("data", t, 8)


@pytest.mark.parametrize("name, need, align", KINDS, ids=IDS)
def test_rejects_other_device(name, need, align):
    with pytest.raises(ValueError, match=f"{name} is on device 1"):
        check(name, FakeTensor(need + 64, BASE, device=1), need, 0, align)
    check(name, FakeTensor(need + 64, BASE, device=1), need, 1, align)
    check(name, FakeTensor(need + 64, BASE, device=1), need, None, align)  # a one-shot on the tensor's device


@pytest.mark.parametrize("name, need, align", KINDS, ids=IDS)
def test_rejects_non_contiguous(name, need, align):
    with pytest.raises(ValueError, match=f"{name} must be contiguous"):
        check(name, FakeTensor(4 * need + 64, BASE, contiguous=False), need, 0, align)


@pytest.mark.parametrize("name, need, align", [k for k in KINDS if k[1]], ids=[i for i, k in zip(IDS, KINDS) if k[1]])
def test_rejects_too_small(name, need, align):
    with pytest.raises(ValueError, match=f"{name} buffer too small"):
        check(name, FakeTensor(need - 1, BASE), need, 0, align)
    with pytest.raises(ValueError, match=f"{name} buffer too small"):
        check(name, FakeTensor(0, BASE), need, 0, align)


@pytest.mark.parametrize("name, need, align", [k for k in KINDS if k[2] > 1],
                         ids=[i for i, k in zip(IDS, KINDS) if k[2] > 1])
def test_rejects_misaligned_pointer(name, need, align):
    """Every offset below the alignment but 0, and in particular alignment / 2 and 4."""
    for off in sorted({1, align // 2, align - 1} | ({4} if align > 4 else set())):
        with pytest.raises(ValueError, match=f"{name} must be {align}-byte aligned"):
            check(name, FakeTensor(need + 64, BASE + off), need, 0, align)
    assert check(name, FakeTensor(need + 64, BASE + align), need, 0, align).value == BASE + align


def test_accepts_pointer_at_a_storage_offset():
    """Data may begin anywhere; a digest view may begin at any multiple of its alignment (a row
    slice pool[4:4 + n] of 32-byte rows is at +128: a multiple of 16 and not of 256)."""
    for off in (1, 3, 13):
        assert check("data", FakeTensor(1000, BASE + off), 1000, 0).value == BASE + off
    assert check("digests", FakeTensor(32 * 16, BASE + 128), 32 * 16, 0, 16).value == BASE + 128
    assert check("digests", FakeTensor(20 * 16, BASE + 80), 20 * 16, 0, 4).value == BASE + 80
    assert check("crcs", FakeTensor(8 * 16, BASE + 32), 8 * 16, 0, 8).value == BASE + 32


def test_element_type_does_not_matter():
    """int32- and uint8-typed buffers of the same bytes are the same to the kernels."""
    assert check("data", FakeTensor(1000, BASE, itemsize=4), 1000, 0).value == BASE
    assert check("data", FakeTensor(1000, BASE, itemsize=1), 1000, 0).value == BASE
    assert check("digests", FakeTensor(512, BASE, itemsize=1), 512, 0, 16).value == BASE
    with pytest.raises(ValueError, match="data buffer too small"):
        check("data", FakeTensor(996, BASE, itemsize=4), 1000, 0)


def test_accepts_empty_buffer_when_nothing_is_needed():
    """Stream.update_device with every chunk empty may pass an empty tensor: a null pointer."""
    assert check("data", FakeTensor(0, BASE), 0, 0).value is None


def test_raw_pointer_passes_only_where_the_wrapper_allows_it():
    """The chunk plan's launches take raw device pointers (ints): handed to the library as they
    are, which checks their alignment itself.  Everywhere else an int is not a tensor."""
    assert check("out", BASE + 4, 64, 0, 16, raw=True).value == BASE + 4
    with pytest.raises(ValueError, match="out must be a device tensor"):
        check("out", BASE, 64, 0, 16)


def test_digest_alignment_per_algorithm():
    from s3client_amd import _native
    assert [hashing._digest_align(_native.ALGO_IDS[a]) for a in ("sha256", "md5", "sha1")] == [16, 16, 4]


# ------------------------------------------------------------------ no wrapper goes round it
# Host-side helpers that read a HOST tensor's address; they hand nothing to a device entry point.
HOST_ONLY = {"BufferParts.__init__", "mem_node"}


def _data_ptr_readers(tree) -> set:
    """Qualified names of the functions of hashing.py that mention `.data_ptr`."""
    found = set()

    def walk(node, scope):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.FunctionDef, ast.ClassDef)):
                walk(child, scope + [child.name])
            else:
                if isinstance(child, ast.Attribute) and child.attr == "data_ptr":
                    found.add(".".join(scope))
                walk(child, scope)

    walk(tree, [])
    return found


def test_only_the_validator_reads_a_device_tensors_pointer():
    """Every `<tensor>.data_ptr()` of hashing.py is inside _device_buffer (or one of the two
    host-memory helpers), so no `ctypes.c_void_p(<tensor>.data_ptr())` can reach lib() without
    the checks: a wrapper added later cannot skip them."""
    src = inspect.getsource(hashing)
    assert _data_ptr_readers(ast.parse(src)) == {"_device_buffer"} | HOST_ONLY
    # and the reader notices a wrapper that does it
    bad = src + "\ndef later(t):\n    return lib().s3h_x(ctypes.c_void_p(t.data_ptr()))\n"
    assert "later" in _data_ptr_readers(ast.parse(bad))

