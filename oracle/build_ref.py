"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Stages the reference's own Python sources (the upstream vit_tensorflow package) into oracle/_ref/vit_tensorflow/, so that what runs
them -- oracle/gen_ref_fixtures.py and the tests of tests/test_ref_fixtures.py that re-execute the reference under oracle/tf_shim --
reads them from inside the repository tree.  oracle/_ref/ is git-ignored: nothing of the reference is ever committed.

    python -m oracle.build_ref          # (also run by __graft_entry__.build())

The source is VITX_REFERENCE_DIR when set, else the reference checkout's usual place.  Where there is no such directory the stage
is a no-op and the tests that need it skip with that reason; a directory that exists but cannot be staged in full is an error.
"""
from __future__ import annotations

import filecmp
import os
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "vit_tensorflow")
DEFAULT_SOURCE = "/root/reference/vit_tensorflow"


def source_dir() -> str:
    return os.environ.get("VITX_REFERENCE_DIR") or DEFAULT_SOURCE


def stage() -> str | None:
    """Copy the reference's *.py files into oracle/_ref/vit_tensorflow/ (files whose content is unchanged are left alone).
    Returns the staged directory, or None when there is no reference directory here; raises when one exists but cannot be staged."""
    src = source_dir()
    if not os.path.isdir(src):
        return None
    names = sorted(f for f in os.listdir(src) if f.endswith(".py"))
    if not names:
        raise RuntimeError(f"{src} holds no Python sources: not a checkout of the reference's vit_tensorflow package")
    os.makedirs(STAGED, exist_ok=True)
    try:
        for f in names:
            s, d = os.path.join(src, f), os.path.join(STAGED, f)
            if not (os.path.exists(d) and filecmp.cmp(s, d, shallow=False)):
                shutil.copyfile(s, d)
    except OSError as ex:   # no partial copy is left behind for the tests to half-run on
        shutil.rmtree(STAGED, ignore_errors=True)
        raise RuntimeError(f"staging the reference's sources from {src} failed: {ex}") from ex
    for f in os.listdir(STAGED):   # a file the reference no longer has must not keep importing
        if f.endswith(".py") and f not in names:
            os.remove(os.path.join(STAGED, f))
    return STAGED


if __name__ == "__main__":
    print(stage() or f"no reference sources at {source_dir()}: nothing staged")
