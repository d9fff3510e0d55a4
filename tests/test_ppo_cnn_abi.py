"""sgk_ppo_cnn_learner (include/sgk.h) and _lib.SgkPpoCnnLearner have the same layout: a C program compiled against the header prints
sizeof and every field's offsetof, and they must equal the ctypes structure's. A mismatch would otherwise only show on the GPU, as a
pointer in the wrong field."""
import os
import shutil
import subprocess

import pytest

from safe_grid_agents_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    fields = [f for f, _ in _lib.SgkPpoCnnLearner._fields_]
    src = ["#include <stddef.h>", "#include <stdio.h>", '#include "sgk.h"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(sgk_ppo_cnn_learner));']
    src += ['  printf("%s %%zu\\n", offsetof(sgk_ppo_cnn_learner, %s));' % (f, f) for f in fields]
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_ppo_cnn_learner_layout_matches_the_header(tmp_path):
    got = _c_layout(tmp_path)
    S = _lib.SgkPpoCnnLearner
    assert got["sizeof"] == __import__("ctypes").sizeof(S)
    for name, _ in S._fields_:
        assert got[name] == getattr(S, name).offset, name


def test_ppo_cnn_learner_arrays_have_the_header_lengths():
    S = _lib.SgkPpoCnnLearner
    f = dict(S._fields_)
    assert f["params"]._length_ == 14 and f["m"]._length_ == 14 and f["v"]._length_ == 14
    assert f["old_params"]._length_ == 10
    assert "sgk_ppo_cnn_epochs" in _lib.EXPORTED_SYMBOLS and "sgk_ppo_cnn_workspace_bytes" in _lib.EXPORTED_SYMBOLS
