"""CPU checks of the extension headers (include/freesplat_ext_*.h, _lib.EXTENSION_HEADERS): what tests/test_abi.py holds the
eleven freesplat_amd*.h headers to, for every record added after them (no compute calls here)."""
import ctypes
import itertools
import os
import re

import pytest

from freesplat_amd import _lib
from util_abi import INCLUDE, declared_names, header_text


def _bare_library():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_the_extension_registry_names_every_extension_header_once():
    files = [h.file for h in _lib.EXTENSION_HEADERS]
    assert sorted(files) == sorted(f for f in os.listdir(INCLUDE) if f.startswith("freesplat_ext_") and f.endswith(".h"))
    assert len(set(files)) == len(files) >= 1
    # every header under include/ is in one of the two registries
    assert sorted(files + [h.file for h in _lib.HEADERS]) == sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
    everything = _lib.HEADERS + _lib.EXTENSION_HEADERS
    for a, b in itertools.combinations(everything, 2):
        assert not set(a.signatures) & set(b.signatures), (a.file, b.file)
    assert len({h.version_fn for h in everything}) == len({h.macro for h in everything}) == len({h.label for h in everything}) == len(everything)
    ray = _lib.EXTENSION_HEADERS[0]
    assert ray.file == "freesplat_ext_raycast.h" and ray.label == "ray-cast API"
    assert ray.signatures is _lib.RAYCAST_SIGNATURES and ray.revision == _lib.RAYCAST_API_VERSION == 1 and len(ray.signatures) == 2


@pytest.mark.parametrize("h", _lib.EXTENSION_HEADERS, ids=lambda h: h.file)
def test_every_extension_header_is_exported_bound_and_at_its_revision(h):
    L = _bare_library()
    names = declared_names(h.file)
    assert names and h.version_fn in names
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/{h.file} but not exported"
    assert set(names) == set(h.signatures)
    assert re.search(rf"#define\s+{h.macro}\s+{h.revision}\b", header_text(h.file))
    assert getattr(L, h.version_fn)() == h.revision == getattr(_lib.lib(), h.version_fn)()


MISMATCH = {
    "freesplat_ext_raycast.h": "{lib} has ray-cast API revision 1, this binding expects 2 (include/freesplat_ext_raycast.h "
                               "FS_RAYCAST_API_VERSION): rebuild the library",
}


@pytest.mark.parametrize("i", range(len(_lib.EXTENSION_HEADERS)), ids=lambda i: _lib.EXTENSION_HEADERS[i].file)
def test_a_library_at_another_extension_revision_is_refused_and_not_cached(i, monkeypatch):
    _bare_library()
    ext = _lib.EXTENSION_HEADERS
    h = ext[i]
    monkeypatch.setattr(_lib, "EXTENSION_HEADERS", ext[:i] + (h._replace(revision=h.revision + 1),) + ext[i + 1:])
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.FreeSplatHipError) as e:
        _lib.lib()
    assert str(e.value) == MISMATCH[h.file].format(lib=_lib.LIB_PATH)
    assert _lib._lib is None


def test_a_mismatch_among_the_eleven_is_reported_before_an_extension(monkeypatch):
    """lib() checks HEADERS first, then EXTENSION_HEADERS: with both at a wrong revision the message names the pinned header."""
    _bare_library()
    h, x = _lib.HEADERS[-1], _lib.EXTENSION_HEADERS[0]
    monkeypatch.setattr(_lib, "HEADERS", _lib.HEADERS[:-1] + (h._replace(revision=h.revision + 1),))
    monkeypatch.setattr(_lib, "EXTENSION_HEADERS", (x._replace(revision=x.revision + 1),) + _lib.EXTENSION_HEADERS[1:])
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.FreeSplatHipError, match=re.escape(f"include/{h.file} {h.macro}")):
        _lib.lib()
    assert _lib._lib is None
