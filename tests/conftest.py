import os
import sys

import pytest

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO_ROOT not in sys.path:
    sys.path.insert(0, REPO_ROOT)


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test needs a real MI355X GPU (run via gpurun)"
    )


GOLDEN_DIR = os.path.join(REPO_ROOT, "tests", "golden")
GOLDEN_DATA = os.path.join(GOLDEN_DIR, "data")


def _load_answers():
    import json

    with open(os.path.join(GOLDEN_DIR, "answers.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="session", autouse=True)
def golden_data():
    """The parquet inputs behind tests/golden/answers.json. Several exceed
    the size limit for a committed file, so they are not in git: the seeded
    generator (datagen.gen) reproduces them from GOLDEN_FIXTURES, the same
    way scripts/gen_golden.py wrote them when the answers were recorded.
    Generated once per checkout (tests/golden/data is ignored) into a
    sibling directory and renamed into place, so an interrupted or
    concurrent run never leaves a half-written tree behind."""
    import shutil
    import tempfile

    from datagen.gen import gen_stream
    from tests.golden_queries import GOLDEN_FIXTURES

    manifest = _load_answers()["fixtures"]
    wanted = [os.path.join(GOLDEN_DATA, f)
              for fx in manifest.values() for f in fx["files"]]
    if all(os.path.exists(f) for f in wanted):
        return GOLDEN_DATA
    tmp = tempfile.mkdtemp(prefix="data.gen.", dir=GOLDEN_DIR)
    try:
        for name, params in GOLDEN_FIXTURES.items():
            info = gen_stream(tmp, name, **params)
            rel = [os.path.relpath(f, tmp) for f in info["files"]]
            assert rel == manifest[name]["files"], (
                f"datagen no longer reproduces fixture {name}: "
                "rerun scripts/gen_golden.py")
        if os.path.isdir(GOLDEN_DATA):
            shutil.rmtree(GOLDEN_DATA)  # incomplete leftover
        os.chmod(tmp, 0o755)  # mkdtemp makes it private
        try:
            os.rename(tmp, GOLDEN_DATA)
        except OSError:
            if not all(os.path.exists(f) for f in wanted):
                raise  # otherwise a concurrent run got there first
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return GOLDEN_DATA


@pytest.fixture(scope="session")
def golden(golden_data):
    """Committed golden answers over the generated fixtures:
    {'fixtures': {...}, 'answers': {...}}, with file paths resolved to
    absolute."""
    g = _load_answers()
    gdir = golden_data
    for fx in g["fixtures"].values():
        fx["files"] = [os.path.join(gdir, f) for f in fx["files"]]
    return g
