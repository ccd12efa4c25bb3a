"""The in-tree HIP library resolves every one of its own symbols (a declared-but-undefined
launcher links fine into a shared object and only fails when ctypes loads it on the GPU box)."""
import os
import shutil
import subprocess

import pytest

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rocalphago_amd",
                  "_hipkernels.so")


@pytest.mark.skipif(not os.path.exists(SO) or shutil.which("nm") is None,
                    reason="HIP library not built here")
def test_hip_library_has_no_undefined_own_symbols():
    out = subprocess.run(["nm", "-D", "--undefined-only", SO], stdout=subprocess.PIPE,
                         text=True, check=True).stdout
    # strong undefined symbols of our own code: launchers (rag_*) and anything in an anonymous
    # namespace (_GLOBAL__N_), e.g. an extern declared inside one
    own = [ln for ln in out.splitlines()
           if ("rag_" in ln or "_GLOBAL__N_" in ln) and not ln.strip().startswith("w ")]
    assert not own, own


@pytest.mark.skipif(not os.path.exists(SO), reason="HIP library not built here")
def test_hip_library_loads_with_every_symbol_bound():
    """dlopen with RTLD_NOW (what the GPU box's ctypes load does) binds every reference."""
    import ctypes
    ctypes.CDLL(SO, mode=os.RTLD_NOW | os.RTLD_LOCAL)


@pytest.mark.skipif(not os.path.exists(SO) or shutil.which("nm") is None,
                    reason="HIP library not built here")
def test_exported_symbols_are_the_ctypes_table():
    """The library exports exactly the rag_* entry points ops/_abi.py declares: a name missing
    from the table would be called untyped (pointers truncated to int)."""
    from rocalphago_amd.ops import _abi
    out = subprocess.run(["nm", "-D", "--defined-only", SO], stdout=subprocess.PIPE,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("rag_")}
    assert exported == set(_abi.SIGNATURES)


API_H = os.path.join(os.path.dirname(SO), "..", "csrc", "hip", "rag_api.h")


def _kind(ctype):
    """Argument / return kind of one C type in rag_api.h as its ctypes class."""
    import ctypes
    ctype = " ".join(ctype.replace("const", " ").split())
    if ctype.endswith("*") or ctype == "hipStream_t":
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float,
            "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "long": ctypes.c_long}[ctype]


@pytest.mark.skipif(not os.path.exists(SO), reason="HIP library not built here")
def test_ctypes_signatures_match_the_header():
    """Argument count, every argument's kind and the return kind of each prototype in
    csrc/hip/rag_api.h (which the compiler checks against the definitions) agree with
    _abi.SIGNATURES / RESTYPES."""
    import ctypes
    import re
    from rocalphago_amd.ops import _abi
    with open(API_H) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    protos = re.findall(r"RAG_API\s+(\w+)\s+(rag_\w+)\s*\(([^)]*)\)\s*;", text)
    assert len(protos) == text.count("RAG_API")  # every declaration parsed
    seen = {}
    for ret, name, args in protos:
        assert name not in seen, name
        # "const float* bias" -> type "const float*" (the last word is the parameter's name)
        kinds = [_kind(a.strip().rsplit(None, 1)[0]) for a in args.split(",") if a.strip()]
        seen[name] = (kinds, _kind(ret))
    assert set(seen) == set(_abi.SIGNATURES)
    for name, (kinds, ret) in seen.items():
        assert kinds == list(_abi.SIGNATURES[name]), name
        assert ret is _abi.RESTYPES.get(name, ctypes.c_int), name
