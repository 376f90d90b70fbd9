"""The Python binding's single description of each layout result (tekken-rs_amd _LayoutResult.OUTPUTS / COUNTS and the ctypes
structs) held against the C structs of include/tekken_hip.h.  No GPU: the header is parsed as text."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ["dense", "seqpack", "join", "window", "rowfit"]


def header_members(name):
    """[(member, is_pointer)] of `typedef struct tk_<name> { ... }` in the order of the declaration; a type other than a pointer or
    uint64_t fails: the sizes below know no other."""
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    m = re.search(r"typedef struct tk_%s\s*\{(.*?)\}\s*tk_%s\s*;" % (name, name), hdr, re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = [d.strip() for d in decl.split(",")]
        base, ident = re.match(r"^(.*?)(\**\s*\w+)$", first).groups()
        base_ptr = base.strip().endswith("*")
        base_type = base.replace("*", "").strip()
        for d in [ident] + rest:
            ptr = base_ptr or d.startswith("*")
            assert ptr or base_type == "uint64_t", (name, decl)
            out.append((d.replace("*", "").strip(), ptr))
    return out


@pytest.mark.parametrize("name", PASSES)
def test_result_class_declares_the_header_struct(tk, name):
    R = getattr(tk, name.capitalize() + "Result")
    members = header_members(name)
    assert R.PASS == name
    assert [o[0] for o in R.OUTPUTS] == [m for m, ptr in members if ptr]
    assert list(R.COUNTS) == [m for m, ptr in members if not ptr]
    # the pointers come first in every struct, so no padding: the size is the sum of the members
    assert [ptr for _, ptr in members] == sorted((ptr for _, ptr in members), reverse=True)
    assert ctypes.sizeof(R.STRUCT) == sum(ctypes.sizeof(ctypes.c_void_p) if ptr else 8 for _, ptr in members)
    assert [f[0] for f in R.STRUCT._fields_] == [m for m, _ in members]
    for (_, ptr), (_, ctype) in zip(members, R.STRUCT._fields_):
        assert ctype is (ctypes.c_void_p if ptr else ctypes.c_uint64)


@pytest.mark.parametrize("name", PASSES)
def test_result_attributes_and_views_follow_the_declaration(tk, name):
    R = getattr(tk, name.capitalize() + "Result")
    st = R.STRUCT()
    for i, (field, _) in enumerate(R.STRUCT._fields_):
        setattr(st, field, 0x1000 * (i + 1) if field in [o[0] for o in R.OUTPUTS] else i + 2)
    first_optional = next(o[0] for o in R.OUTPUTS if o[4])
    setattr(st, first_optional, None)
    r = R(st, R.I64, 5) if name != "join" else R(st)
    assert hasattr(r, "typestr") == (name != "join") and hasattr(r, "n_docs") == (name in ("dense", "window", "rowfit"))
    views = r.views()
    assert len(views) == len(R.OUTPUTS)
    for (out, typestr, shape, _, optional), v in zip(R.OUTPUTS, views):
        if out == first_optional:
            assert getattr(r, out + "_ptr") is None and v is None
            continue
        assert getattr(r, out + "_ptr") == getattr(st, out)
        cai = v.__cuda_array_interface__
        assert cai["data"][0] == getattr(st, out) and cai["shape"] == tuple(shape(r))
        assert cai["typestr"] == (typestr or "<i8")
    for k in R.COUNTS:
        assert getattr(r, k) == getattr(st, k)
    assert set(r._counts()) == set(R.DICT_COUNTS) <= set(R.COUNTS) and hasattr(r, "counts") == (name == "rowfit")
