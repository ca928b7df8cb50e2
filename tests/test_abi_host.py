"""The ctypes binding held to the header, once and whole (no GPU, ``_abi.lib()`` is never called): ``_abi.SIGNATURES`` declares exactly
the ``PTX_API`` prototypes of include/proxyt.h, and every argument and return value is of the header's KIND -- a pointer, a signed or
unsigned integer of the header's size, ``float`` or ``double``.  A ``c_int`` bound where the header says ``long``, or a ``c_float``
where it says ``double``, passes every count of arguments and corrupts the call.

Not covered here: what a pointer points to, and the field layouts of the structs that cross the ABI (``PtxShape``, ``PtxWeights``,
``PtxTrainStep``, ...) -- tests/test_host_cpu.py holds those to the compiler's offsets."""
import ctypes

from proxytransformation_amd import _abi
from tests.util import header_prototypes

POINTER = ("pointer",)
C_KINDS = {"int": ("signed", 4), "int32_t": ("signed", 4),
           "long": ("signed", 8), "int64_t": ("signed", 8), "long long": ("signed", 8),
           "size_t": ("unsigned", 8), "uint64_t": ("unsigned", 8), "unsigned long long": ("unsigned", 8),
           "float": ("float", 4), "double": ("float", 8)}


def c_kind(decl: str, named: bool):
    """The kind of a C declaration: a parameter (``named``: its last word is its name, which the header always gives) or a return type."""
    if "*" in decl or "[" in decl:
        return POINTER
    words = [w for w in decl.split() if w != "const"]
    ctype = " ".join(words[:-1] if named else words)
    assert ctype in C_KINDS, f"include/proxyt.h: {decl!r} is of a C type this test has no kind for; add it to C_KINDS"
    return C_KINDS[ctype]


def ctypes_kind(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return POINTER
    if t in (ctypes.c_float, ctypes.c_double):
        return ("float", ctypes.sizeof(t))
    assert issubclass(t, ctypes._SimpleCData) and t._type_ in "bBhHiIlLqQ", f"{t} is of a ctypes type this test has no kind for"
    return ("signed" if t(-1).value < 0 else "unsigned", ctypes.sizeof(t))


def test_kinds_tell_apart_what_a_count_of_arguments_cannot():
    assert ctypes_kind(ctypes.c_int) != ctypes_kind(ctypes.c_long) == c_kind("long n", True) == c_kind("int64_t", False)
    assert ctypes_kind(ctypes.c_float) != ctypes_kind(ctypes.c_double) == c_kind("double eps", True)
    assert ctypes_kind(ctypes.c_size_t) == c_kind("const size_t ws_bytes", True) != ctypes_kind(ctypes.c_int64)
    assert ctypes_kind(ctypes.POINTER(_abi.PtxShape)) == ctypes_kind(ctypes.c_void_p) == c_kind("const PtxShape *s", True)
    assert c_kind("const int32_t ends[]", True) == c_kind("const char *", False) == ctypes_kind(ctypes.c_char_p) == POINTER


def test_the_binding_declares_the_headers_prototypes_and_no_others():
    protos = header_prototypes()
    assert len(protos) >= 166
    assert set(protos) == set(_abi.SIGNATURES), sorted(set(protos) ^ set(_abi.SIGNATURES))


def test_every_argument_and_return_value_is_of_the_headers_kind():
    bad = []
    for name, (result, params) in header_prototypes().items():
        restype, argtypes = _abi.SIGNATURES[name]
        if len(argtypes) != len(params):
            bad.append(f"{name}: {len(params)} parameters in the header, {len(argtypes)} bound")
            continue
        if (restype is None) != (result == "void") or (restype is not None and ctypes_kind(restype) != c_kind(result, False)):
            bad.append(f"{name}: returns {result!r} in the header, bound as {restype}")
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            if ctypes_kind(t) != c_kind(decl, True):
                bad.append(f"{name}: argument {i} is {decl!r} in the header, bound as {t.__name__}")
    assert not bad, "\n".join(bad)
