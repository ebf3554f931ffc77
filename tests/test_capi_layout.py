"""Every ctypes mirror in hslabs_amd/capi.py has the layout the C compiler gives the struct of
include/hslabs.h it stands for (CPU, no library loaded). The structs carry raw device pointers into
the kernels: a field the header gains and the mirror does not, or gains elsewhere, would shift every
pointer behind it. A generated C99 program prints sizeof and offsetof from the header; the mirrors
must agree field by field, and every struct of the header must have a mirror."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

from hslabs_amd import capi

HEADER = os.path.join(ROOT, "include", "hslabs.h")


def header_structs():
    """names of the header's anonymous `typedef struct { ... } hs_*;`"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.findall(r"typedef\s+struct\s*\{[^{}]*\}\s*(hs_\w+)\s*;", src)


def c_layouts(tmp_path):
    """{struct: (sizeof, {field: (offsetof, sizeof)})} as gcc lays out include/hslabs.h, for the fields
    the mirrors name"""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "hslabs.h"', "int main(void) {"]
    for cname, cls in capi.C_STRUCTS.items():
        lines.append(f'  printf("{cname} - %zu 0\\n", sizeof({cname}));')
        for field in cls._fields_:
            f = field[0]
            lines.append(f'  printf("{cname} {f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));')
    lines += ["  return 0;", "}", ""]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    res = {}
    for ln in out.splitlines():
        cname, f, a, b = ln.split()
        if f == "-":
            res[cname] = (int(a), {})
        else:
            res[cname][1][f] = (int(a), int(b))
    return res


def test_every_header_struct_has_a_mirror():
    declared = header_structs()
    assert len(declared) >= 15 and len(set(declared)) == len(declared), declared
    assert sorted(capi.C_STRUCTS) == sorted(declared)
    mirrors = [v for v in vars(capi).values() if isinstance(v, type) and issubclass(v, ctypes.Structure)
               and v is not ctypes.Structure]
    assert len(mirrors) == len(capi.C_STRUCTS)
    assert set(mirrors) == set(capi.C_STRUCTS.values())  # no mirror without a C name, none named twice


def test_mirrors_have_the_headers_layout(tmp_path):
    want = c_layouts(tmp_path)
    n_fields = 0
    for cname, cls in capi.C_STRUCTS.items():
        size, fields = want[cname]
        assert ctypes.sizeof(cls) == size, f"{cls.__name__}: sizeof {ctypes.sizeof(cls)}, {cname} has {size}"
        assert len(fields) == len(cls._fields_), f"{cls.__name__}: a field is named twice"
        for field in cls._fields_:
            d = getattr(cls, field[0])
            assert (d.offset, d.size) == fields[field[0]], \
                f"{cls.__name__}.{field[0]}: (offset, size) {(d.offset, d.size)}, {cname} has {fields[field[0]]}"
            n_fields += 1
        # the fields tile the struct up to alignment padding: the header has none the mirror lacks
        end = max(o + s for o, s in fields.values())
        assert size - end < ctypes.alignment(cls), f"{cname}: {size - end} bytes after the mirror's last field"
    assert n_fields >= 178
