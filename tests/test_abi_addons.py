"""CPU checks of the add-on headers (include/ext/<name>.h, _lib.ADDON_HEADERS): what tests/test_abi.py holds the eleven
freesplat_amd*.h headers to and tests/test_abi_extensions.py the extension headers, for every record added from now on (no compute
calls here).  This file is generic: it is parametrised over the tuple, forms every expected value from the record's own fields
and pins no count, no table size and no revision -- a further record passes it unchanged."""
import ctypes
import itertools
import os
import re

import pytest

from freesplat_amd import _lib
from util_abi import INCLUDE, declared_names, header_text

ADDONS = _lib.ADDON_HEADERS
BY_FILE = lambda h: h.file


def _bare_library():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def _mismatch(h, got, expected):
    """The message lib() raises for header `h`, from the record's own fields."""
    return (f"{_lib.LIB_PATH} has {h.label} revision {got}, this binding expects {expected} (include/{h.file} {h.macro}): "
            "rebuild the library")


def test_the_addon_registry_names_every_header_under_ext_once():
    files = [h.file for h in ADDONS]
    under_ext = sorted("ext/" + f for f in os.listdir(os.path.join(INCLUDE, "ext")) if f.endswith(".h"))
    assert sorted(files) == under_ext
    assert len(set(files)) == len(files) >= 1
    assert all(isinstance(h, _lib.Header) for h in ADDONS)
    everything = _lib.HEADERS + _lib.EXTENSION_HEADERS + ADDONS
    for a, b in itertools.combinations(everything, 2):
        assert not set(a.signatures) & set(b.signatures), (a.file, b.file)
    for field in ("file", "version_fn", "macro", "label"):
        assert len({getattr(h, field) for h in everything}) == len(everything), field
    # the Makefile rebuilds the library when an add-on header changes
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    for f in files:
        assert f"../../include/{f}" in makefile, f


@pytest.mark.parametrize("h", ADDONS, ids=BY_FILE)
def test_every_addon_header_is_exported_bound_and_at_its_revision(h):
    L = _bare_library()
    names = declared_names(h.file)
    assert names and h.version_fn in names
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/{h.file} but not exported"
    assert set(names) == set(h.signatures)
    assert re.search(rf"#define\s+{h.macro}\s+{h.revision}\b", header_text(h.file))
    assert getattr(L, h.version_fn)() == h.revision == getattr(_lib.lib(), h.version_fn)()
    bound = getattr(_lib.lib(), h.version_fn)
    assert bound.restype is h.signatures[h.version_fn][0] and list(bound.argtypes) == h.signatures[h.version_fn][1]


@pytest.mark.parametrize("i", range(len(ADDONS)), ids=lambda i: ADDONS[i].file)
def test_a_library_at_another_addon_revision_is_refused_and_not_cached(i, monkeypatch):
    _bare_library()
    h = ADDONS[i]
    monkeypatch.setattr(_lib, "ADDON_HEADERS", ADDONS[:i] + (h._replace(revision=h.revision + 1),) + ADDONS[i + 1:])
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.FreeSplatHipError) as e:
        _lib.lib()
    assert str(e.value) == _mismatch(h, h.revision, h.revision + 1)
    assert _lib._lib is None


@pytest.mark.parametrize("registry", ["HEADERS", "EXTENSION_HEADERS"])
@pytest.mark.parametrize("i", range(len(ADDONS)), ids=lambda i: ADDONS[i].file)
def test_a_mismatch_in_a_closed_registry_is_reported_before_an_addon(i, registry, monkeypatch):
    """lib() checks HEADERS, then EXTENSION_HEADERS, then ADDON_HEADERS: with an add-on and the last record of a closed registry
    both at a wrong revision, the message names the closed registry's header."""
    _bare_library()
    closed = getattr(_lib, registry)
    h, x = closed[-1], ADDONS[i]
    monkeypatch.setattr(_lib, registry, closed[:-1] + (h._replace(revision=h.revision + 1),))
    monkeypatch.setattr(_lib, "ADDON_HEADERS", ADDONS[:i] + (x._replace(revision=x.revision + 1),) + ADDONS[i + 1:])
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.FreeSplatHipError) as e:
        _lib.lib()
    assert str(e.value) == _mismatch(h, h.revision, h.revision + 1)
    assert _lib._lib is None
