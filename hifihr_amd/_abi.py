"""The C ABI as a table: every prototype of include/hifihr.h with its ctypes signature.

`HifihrLib` binds `argtypes` and `restype` from this table, so the header is the only place a signature is written down.
The parser is strict on purpose: a prototype it skipped, or a type it guessed, would hand a kernel a wild pointer or a truncated size.
"""
from __future__ import annotations

import functools
import os
import re
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_long, c_size_t, c_void_p

from ._lib import HifihrError, _LinearDesc

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hifihr.h"))

_BY_VALUE = {"int": c_int, "float": c_float, "long": c_long, "size_t": c_size_t}
_RETURNS = {("int", 0): c_int, ("size_t", 0): c_size_t, ("long", 0): c_long, ("char", 1): c_char_p, ("void", 0): None}
_POINTERS = {("float", 1): POINTER(c_float), ("int32_t", 1): POINTER(c_int32), ("int", 1): POINTER(c_int32), ("char", 1): c_char_p,
             ("float", 2): POINTER(POINTER(c_float)), ("hifihr_linear_desc", 1): POINTER(_LinearDesc)}


def _split(ctype):
    """'const float* const*' -> ('float', 2): the type without its qualifiers, and its pointer depth."""
    return " ".join(re.sub(r"\bconst\b|\*", " ", ctype).split()), ctype.count("*")


def _param(ctype, handles, where):
    base, depth = _split(ctype)
    if depth == 0 and base in _BY_VALUE:
        return _BY_VALUE[base]
    if (base, depth) in _POINTERS:
        return _POINTERS[base, depth]
    if depth == 2 and base in handles:
        return POINTER(c_void_p)               # where a create call stores the handle
    if depth == 1:
        return c_void_p                        # an untyped address: void*, a handle, a stream, a buffer of another element type
    raise HifihrError(f"{where}: no ctypes rule for the parameter type '{ctype.strip()}'")


def _return(ctype, handles, where):
    key = _split(ctype)
    if key in _RETURNS:
        return _RETURNS[key]
    if key[1] == 1 and key[0] in handles:
        return c_void_p
    raise HifihrError(f"{where}: no ctypes rule for the return type '{ctype.strip()}'")


def _parse(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    loose = set(re.findall(r"\b(hifihr_[a-z0-9_]+)\s*\(", text))          # what tests/test_abi.py takes for the declared names
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    handles = set(re.findall(r"\btypedef\s+struct\s+\w+\s+(\w+)\s*;", text))
    text = re.sub(r"\btypedef\s+struct\s+\w+\s+\w+\s*;|\btypedef\s+struct\s*\w*\s*\{[^{}]*\}\s*\w+\s*;", " ", text)
    text = re.sub(r'\bextern\s+"C"\s*\{|^\s*\}\s*$', " ", text, flags=re.M)
    table = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\b(hifihr_[a-z0-9_]+) ?\(([^()]*)\)", stmt)
        if not m or m[2] in table:
            raise HifihrError(f"include/hifihr.h: not a prototype the binding can read: '{stmt[:120]}'")
        argtypes, argnames = [], []
        for p in ([] if m[3].strip() in ("", "void") else m[3].split(",")):
            pm = re.fullmatch(r"\s*(.*[\s*])(\w+)\s*(\[\d*\])?\s*", p)
            if not pm:
                raise HifihrError(f"{m[2]}: cannot read the parameter '{p.strip()}'")
            argtypes.append(_param(pm[1] + ("*" if pm[3] else ""), handles, m[2]))        # an array parameter is a pointer
            argnames.append(pm[2])
        table[m[2]] = (_return(m[1], handles, m[2]), argtypes, argnames)
    if set(table) != loose:
        raise HifihrError(f"include/hifihr.h: names that are not plain prototypes: {sorted(loose ^ set(table))}")
    return table


@functools.lru_cache(maxsize=None)
def _header_table():
    try:
        with open(HEADER_PATH) as f:
            text = f.read()
    except OSError as e:
        raise HifihrError(f"{HEADER_PATH} not readable ({e}): the ctypes signatures are read from it; there is no fallback table.") from e
    return _parse(text)


def prototypes(header_text=None):
    """name -> (restype, argtypes, argnames) for every prototype of include/hifihr.h (parsed once), or of `header_text`."""
    return _parse(header_text) if header_text is not None else _header_table()
