"""CPU: the C-ABI of the triangle-motif counts (csrc/motifs.hip): every entry is declared in include/pygsd_hip.h, exported by
the built library and bound in _cabi.PROTOTYPES with the header's argument count; bad arguments and entry counts beyond the
int32 CSR limit are refused on the host before any launch."""
import ctypes
import os
import re
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pygsd_motif_workspace", "pygsd_motif_neighbourhoods", "pygsd_motif_count")


def header_arg_counts():
    with open(os.path.join(ROOT, "include", "pygsd_hip.h")) as f:
        text = f.read()
    out = {}
    for m in re.finditer(r"^int (pygsd_motif_\w+)\(([^;]*)\);", text, re.M):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    return out


def in_thread(body):
    """Runs `body` on a thread of its own: the library's error string is thread-local, so the refusals provoked here leave
    the main thread's clean."""
    failures = []

    def run():
        try:
            body()
        except BaseException as exc:    # noqa: B902 -- re-raised on the main thread
            failures.append(exc)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failures:
        raise failures[0]


def test_motif_entries_declared_exported_and_bound():
    from pytorch_geometric_signed_directed_amd import _cabi
    counts = header_arg_counts()
    assert sorted(counts) == sorted(ENTRIES)
    lib = ctypes.CDLL(_cabi.lib_path())
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in _cabi.PROTOTYPES, name
        assert len(_cabi.PROTOTYPES[name][1]) == counts[name], name


def test_motif_arguments_are_checked_without_a_gpu():
    in_thread(_argument_checks)


def _argument_checks():
    from pytorch_geometric_signed_directed_amd import _cabi
    lib = _cabi.lib()
    need = ctypes.c_size_t(0)
    assert lib.pygsd_motif_workspace(5, None) != 0 and b"null pointer" in lib.pygsd_last_error()
    assert lib.pygsd_motif_workspace(-1, ctypes.byref(need)) != 0 and b"negative" in lib.pygsd_last_error()
    assert lib.pygsd_motif_workspace(0, ctypes.byref(need)) == 0 and need.value == 0    # no keys: no workspace
    rc = lib.pygsd_motif_neighbourhoods(None, None, 4, 10, None, None, None, None, 0, None)
    assert rc != 0 and b"null pointer" in lib.pygsd_last_error()
    rc = lib.pygsd_motif_neighbourhoods(None, None, -4, 10, None, None, None, None, 0, None)
    assert rc != 0 and b"negative" in lib.pygsd_last_error()
    rc = lib.pygsd_motif_count(None, 4, 10, None, None, None, None, 4, 0, None, None)
    assert rc != 0 and b"null pointer" in lib.pygsd_last_error()
    rc = lib.pygsd_motif_count(None, 4, -1, None, None, None, None, 4, 0, None, None)
    assert rc != 0 and b"negative" in lib.pygsd_last_error()
    rc = lib.pygsd_motif_count(None, 4, 10, None, None, None, None, 4, 2, None, None)
    assert rc != 0 and b"tier" in lib.pygsd_last_error()
    rc = lib.pygsd_motif_count(None, 4, 10, None, None, None, None, 5, 0, None, None)
    assert rc != 0 and b"ids" in lib.pygsd_last_error()
    assert lib.pygsd_motif_count(None, 0, 10, None, None, None, None, 0, 0, None, None) == 0    # nothing to count
    with pytest.raises(RuntimeError, match="null pointer"):
        _cabi.check(lib.pygsd_motif_workspace(5, None), "pygsd_motif_workspace")


def test_motif_int32_limit_is_named():
    in_thread(_limit_checks)


def _limit_checks():
    from pytorch_geometric_signed_directed_amd import _cabi
    from pytorch_geometric_signed_directed_amd.sparse_gram import check_nnz
    lib = _cabi.lib()
    need = ctypes.c_size_t(0)
    big = 1 << 30                                   # 2^31 typed entries: one beyond the limit
    assert lib.pygsd_motif_workspace(big, ctypes.byref(need)) != 0 and b"2^31 - 1" in lib.pygsd_last_error()
    rc = lib.pygsd_motif_neighbourhoods(None, None, big, 10, None, None, None, None, 0, None)
    assert rc != 0 and b"2^31 - 1" in lib.pygsd_last_error()
    with pytest.raises(RuntimeError, match=r"2\^31 - 1"):
        check_nnz(2 * big, "typed motif neighbourhoods")


def test_motif_constants_and_cpu_refusal():
    """The SDGNN masks partition six counters each; the device entry points refuse host tensors."""
    import torch
    from pytorch_geometric_signed_directed_amd import motifs
    assert len(set(motifs.SDGNN_POS) | set(motifs.SDGNN_NEG)) == 12
    assert not set(motifs.SDGNN_POS) & set(motifs.SDGNN_NEG)
    with pytest.raises(Exception):
        motifs.signed_neighbourhoods(torch.tensor([[0, 1, 1]]), 2)
