"""build.py's source list is the set of translation units in csrc/, and a name in it that does not exist stops the build before a
compiler starts (it used to be skipped, and surfaced as an undefined symbol at link or load time).  No GPU, nothing is compiled."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def build_py():
    spec = importlib.util.spec_from_file_location("e3d_build_under_test", os.path.join(ROOT, "dataset-pipeline_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sources_are_the_hip_files_of_csrc(build_py):
    on_disk = sorted(f for f in os.listdir(build_py.CSRC) if f.endswith(".hip"))
    assert sorted(build_py.SOURCES) == on_disk
    assert len(set(build_py.SOURCES)) == len(build_py.SOURCES)


def test_extra_flags_name_listed_sources(build_py):
    assert set(build_py.EXTRA_FLAGS) <= set(build_py.SOURCES)


def test_missing_source_raises_before_any_compiler_starts(build_py, monkeypatch):
    started = []

    def no_process(cmd, *a, **kw):
        started.append(cmd)
        raise AssertionError("a compiler was started: %r" % (cmd,))

    monkeypatch.setattr(build_py, "SOURCES", list(build_py.SOURCES) + ["e3d_no_such_file.hip"])
    monkeypatch.setattr(build_py.subprocess, "Popen", no_process)
    monkeypatch.setattr(build_py.subprocess, "check_call", no_process)
    with pytest.raises(RuntimeError, match="e3d_no_such_file.hip"):
        build_py.build(force=True)
    assert started == []
