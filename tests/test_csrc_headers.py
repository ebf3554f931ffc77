"""The layout of hslabs_amd/csrc: every header stands alone (it compiles on its own, so what it depends on is what
it includes), no source includes a .hip, and the build's staleness list is the directory's headers."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "hslabs_amd", "csrc")
HEADERS = sorted(f for f in os.listdir(SRC) if f.endswith(".h"))
# the device code of the step kernels, compiled once per precision (hs_kernels.hip, hs_kernels_f32.hip)
STEP_HEADERS = ["hs_step_base.h", "hs_step_kin.h", "hs_step_solve.h", "hs_rollout_kernel.h", "hs_limb.h"]
F32 = ["-DHS_REAL=float", "-DHS_REAL_IS_FLOAT=1"]


def _hipcc():
    from hslabs_amd import build

    try:
        return build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")


def _syntax_only(header, defines=()):
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-x", "hip", *defines,
                        os.path.join(SRC, header)], capture_output=True, text=True)
    assert r.returncode == 0, f"{header} {' '.join(defines)} does not compile on its own:\n{r.stderr[-4000:]}"


def test_step_headers_exist():
    assert set(STEP_HEADERS) <= set(HEADERS)


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header):
    _syntax_only(header)


@pytest.mark.parametrize("header", STEP_HEADERS)
def test_step_header_compiles_alone_f32(header):
    _syntax_only(header, F32)


def test_no_include_of_a_hip():
    bad = []
    for f in sorted(os.listdir(SRC)):
        with open(os.path.join(SRC, f), errors="replace") as fh:
            bad += [f"{f}:{i}: {ln.strip()}" for i, ln in enumerate(fh, 1)
                    if re.match(r'\s*#\s*include\s*["<][^">]*\.hip[">]', ln)]
    assert not bad, bad


def test_build_headers_are_the_directory(tmp_path, monkeypatch):
    from hslabs_amd import build

    want = [os.path.join(SRC, h) for h in HEADERS] + [os.path.join(ROOT, "include", "hslabs.h")]
    got = [os.path.normpath(os.path.join(build.SRC, h)) for h in build.HEADERS]
    assert sorted(got) == sorted(want)
    # found when asked, not when the module was imported: a header added later is watched too
    (tmp_path / "later.h").write_text("#pragma once\n")
    (tmp_path / "unit.hip").write_text("\n")
    monkeypatch.setattr(build, "SRC", str(tmp_path))
    assert [h for h in build.HEADERS if not h.endswith("hslabs.h")] == ["later.h"]
