"""C-ABI surface: the library loads, exports every symbol include/circminer_hot.h declares, and
fails loudly (never falls back to a CPU path) when no HIP device is present."""
import ctypes as C
import os
import re

import pytest

from circminer_amd import _build, lib as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    hdr = open(os.path.join(ROOT, "include", "circminer_hot.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _declared_symbols():
    return sorted(set(re.findall(r"\b(cm_[a-z_]+)\s*\(", _header())))


def _declarations():
    """name -> parameter list (the text between the parentheses) of every function the header declares."""
    out = {}
    for m in re.finditer(r"\b(cm_[a-z_]+)\s*\(", _header()):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(m.string[i], 0)
            i += 1
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = " ".join(m.string[m.end():i - 1].split())
    return out


def _top_level(params):
    """The parameters of a list, split at the commas outside parentheses; `void` and the empty list are none."""
    parts, depth, cur = [], 0, ""
    for ch in params:
        depth += {"(": 1, ")": -1}.get(ch, 0)
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    parts.append(cur.strip())
    return [] if parts in ([""], ["void"]) else parts


def test_header_symbols_exported():
    L = cl.load()
    names = _declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"libcmhot.so does not export {n}"
    assert set(names) == set(cl.EXPORTED_SYMBOLS), set(names) ^ set(cl.EXPORTED_SYMBOLS)


def _host_side_names():
    """The functions the host-only sources define: one build, one definition, no line in the table."""
    csrc = os.path.join(ROOT, "circminer_amd", "csrc")
    names = []
    for f in sorted(os.listdir(csrc)):
        if f.startswith("host_") and f.endswith(".cpp"):
            names += re.findall(r'^(?:extern "C" )?(?:int|void|const char \*) ?(cm_[a-z_]+)\(', open(os.path.join(csrc, f)).read(), flags=re.M)
    assert len(names) == len(set(names))
    return set(names)


def test_table_names_are_the_headers():
    """cm_device_abi.def lists the header's functions that the host-only sources do not define, each once."""
    table = [row[2] for row in _build.device_abi()]
    assert len(table) == len(set(table)) >= 40
    host = _host_side_names()
    assert not set(table) & host, set(table) & host
    assert set(table) | host == set(_declared_symbols()), (set(table) | host) ^ set(_declared_symbols())
    decl = _declarations()
    for _, _, name, params, _ in _build.device_abi():      # "parameter names are the header's": the same text, CM_CTX for the context
        assert params.replace("CM_CTX", "cm_ctx") == decl[name], name


def test_table_arguments_follow_parameters():
    """A CM_DEV line passes `in` and then its parameters in their order (the compiler sees only their number and types)."""
    n = 0
    for macro, _, name, params, args in _build.device_abi():
        if macro == "CM_DEV":
            names = [re.search(r"(\w+)(?:\[\d*\])?$", p).group(1) for p in _top_level(params)]
            assert names[0] == "ctx" and [a.strip() for a in args.split(",")] == ["in"] + names[1:], name
            n += 1
    assert n >= 36
    own = sorted(row[2] for row in _build.device_abi() if row[0] == "CM_DEV_OWN")
    assert own == ["cm_chain_batch", "cm_create", "cm_destroy", "cm_last_error"]


def test_signatures_have_the_headers_arity():
    decl = _declarations()
    assert set(decl) == set(cl.SIGNATURES) and len(decl) >= 84
    for name, params in decl.items():
        assert len(cl.SIGNATURES[name][1]) == len(_top_level(params)), name


def test_null_context_every_wrapper():
    """Every generated wrapper answers a null context itself (CM_EINVAL), whatever else it is given."""
    L = cl.load()
    n = 0
    for macro, ret, name, _, _ in _build.device_abi():
        if macro == "CM_DEV" and ret == "int":
            rest = [0 if issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ" else None for t in cl.SIGNATURES[name][1][1:]]
            assert getattr(L, name)(None, *rest) == -1, name
            n += 1
    assert n >= 36


def test_struct_layouts_match_header():
    assert C.sizeof(cl.MappedRead) == 72 and cl.MAPPED_DTYPE.itemsize == 72
    assert cl.CHAIN_DTYPE.itemsize == 8 + 4 * 16 * 2
    assert C.sizeof(cl.Params) == 48
    assert C.sizeof(cl.DpReq) == cl.DP_REQ_DTYPE.itemsize == 40 and C.sizeof(cl.DpRes) == cl.DP_RES_DTYPE.itemsize == 20      # cm_dp_req, cm_dp_res
    assert C.sizeof(cl.AnnotReq) == cl.ANNOT_REQ_DTYPE.itemsize == 32 and C.sizeof(cl.AnnotRes) == cl.ANNOT_RES_DTYPE.itemsize == 16      # cm_annot_req, cm_annot_res


def test_no_cpu_fallback_without_device():
    import torch
    L = cl.load()
    h = C.c_void_p()
    P = cl.default_params()
    rc = L.cm_create(C.byref(P), C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0
        L.cm_destroy(h)
    else:
        assert rc == -2 and not h          # CM_ENODEV: the hot path is HIP-only
        with pytest.raises(RuntimeError):
            cl.HotPath(P)


def test_bad_params_rejected():
    L = cl.load()
    h = C.c_void_p()
    for kw in (dict(kmer=13), dict(kmer=23), dict(max_chain_len=31), dict(band=9), dict(seed_lim=0)):
        P = cl.default_params(**kw)
        assert L.cm_create(C.byref(P), C.byref(h)) == -1      # CM_EINVAL before any device is touched
    assert L.cm_dp_batch(None, C.byref(cl.default_params()), None, 0, None, 0, 144, 0, 0, 0, None) == -1      # the test hook without a context


def test_product_does_not_reference_oracle():
    """The oracle is test infrastructure: nothing under circminer_amd/ may import, link or call it."""
    for dp, _, fs in os.walk(os.path.join(ROOT, "circminer_amd")):
        for f in fs:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle_py" not in txt and "cm_oracle" not in txt and "libcmoracle" not in txt, f
