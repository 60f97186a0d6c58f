"""Shared helper of the C-boundary tests: the entry points a header under include/ declares."""
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def header_text(header: str) -> str:
    return open(os.path.join(INCLUDE, header)).read()


def declared_names(header: str) -> list:
    """Sorted names of the fs_* functions `header` declares (block comments stripped first: they quote entry points too)."""
    text = re.sub(r"/\*.*?\*/", "", header_text(header), flags=re.S)
    return sorted(set(re.findall(r"\b(fs_[a-z0-9_A-Z]+)\s*\(", text)))
