"""CPU: the built library exports cc_engine_reset_streams, include/cc_hip.h declares it with the documented signature and the Python
face binds it. No compute is called here."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, load_library
    build.build()
    return load_library()


def test_reset_streams_is_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "cc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+cc_engine_reset_streams\s*\(\s*cc_engine\s*\*\s*e\s*,\s*int\s+n\s*,\s*const\s+int\s*\*\s*streams\s*\)\s*;", code)
    assert hasattr(lib, "cc_engine_reset_streams"), "cc_engine_reset_streams is declared in include/cc_hip.h but not exported by libcc_hip.so"
    assert len(lib.cc_engine_reset_streams.argtypes) == 3


def test_engine_has_reset_streams_with_a_docstring():
    from continuous_clustering_amd import Engine
    assert callable(Engine.reset_streams) and Engine.reset_streams.__doc__
