"""nerfactor_amd/build.py on a tree the running user may only read (the tests and bench.py call build() first): an up-to-date
library is returned without creating or opening anything for writing; a stale one is an error that says so."""
import builtins
import os

import pytest


def _read_only(monkeypatch):
    real_open = builtins.open

    def ro_open(path, mode='r', *a, **kw):
        if any(c in mode for c in 'wax+'):
            raise PermissionError(13, 'Permission denied', str(path))
        return real_open(path, mode, *a, **kw)

    def ro_makedirs(path, *a, **kw):
        raise PermissionError(13, 'Permission denied', str(path))
    monkeypatch.setattr(builtins, 'open', ro_open)
    monkeypatch.setattr(os, 'makedirs', ro_makedirs)


def test_an_up_to_date_build_writes_nothing(nfx_lib, monkeypatch):
    from nerfactor_amd import build
    _read_only(monkeypatch)
    assert build.build() == build.LIB


def test_a_stale_build_in_a_read_only_tree_is_an_error(nfx_lib, monkeypatch):
    from nerfactor_amd import build
    monkeypatch.setattr(build, '_headers_mtime', lambda: float('inf'))       # every object older than its headers
    _read_only(monkeypatch)
    with pytest.raises(RuntimeError, match='out of date'):
        build.build()
