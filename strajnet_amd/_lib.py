"""ctypes binding of libstrajnet_hip.so (the C-ABI HIP library).

include/strajnet_hip.h is the single declaration of the ABI: the library's sources compile against it, and this module reads its
prototypes, argument-block structs and enums from it at import (read_header) -- nothing of the ABI is typed a second time here.

The product path has NO CPU fallback: if the library is missing this raises, loudly.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'strajnet_hip.h')
LIB_PATH = os.environ.get('STJ_LIB_PATH') or os.path.join(_HERE, 'libstrajnet_hip.so')     # override: A/B runs of two builds

vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
_SCALARS = {'int': ci, 'long long': cl, 'float': cf, 'uint32_t': ctypes.c_uint32, 'hipStream_t': vp}


class StjError(RuntimeError):
    pass


def _decl(text, where):
    """One declaration `type name` -> (name, ctype): any pointer is c_void_p, a scalar must be in _SCALARS."""
    m = re.fullmatch(r'\s*(.*?)\s*\b(\w+)\s*', text, flags=re.S)
    ty = ' '.join(m.group(1).split()) if m else ''
    if not ty:
        raise StjError(f'{where}: cannot read the declaration {text.strip()!r}')
    if '*' in ty:
        return m.group(2), vp
    if ty not in _SCALARS:
        raise StjError(f'{where}: no ctypes mapping for type {ty!r} in {text.strip()!r}')
    return m.group(2), _SCALARS[ty]


def read_header(text):
    """The C ABI as the header text declares it: (signatures, restypes, structs, enums).
    signatures: name -> argument ctypes and restypes: name -> c_int | c_longlong, of every `int | long long stj_*(...);` prototype;
    structs: name -> ordered ctypes _fields_ of every `typedef struct stj_* {...} stj_*;`; enums: name -> {enumerator: value}."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', '', text, flags=re.S)
    signatures, restypes, structs, enums = {}, {}, {}, {}
    for ret, name, params in re.findall(r'\b(int|long long)\s+(stj_\w+)\s*\(([^()]*)\)\s*;', text):
        params = [] if params.strip() in ('', 'void') else params.split(',')
        signatures[name] = [_decl(p, name)[1] for p in params]
        restypes[name] = _SCALARS[ret]
    for name, body in re.findall(r'\btypedef\s+struct\s+(stj_\w+)\s*\{(.*?)\}\s*\1\s*;', text, flags=re.S):
        fields = structs[name] = []
        for member in filter(str.strip, body.split(';')):
            first, *more = member.split(',')             # `int a, b, c;`: one type, several names
            fields.append(_decl(first, name))
            for n in more:
                if fields[-1][1] is vp or not re.fullmatch(r'\s*\w+\s*', n):
                    raise StjError(f'{name}: cannot read the declarators of {member.strip()!r}')
                fields.append((n.strip(), fields[-1][1]))
    for name, body in re.findall(r'\benum\s+(stj_\w+)\s*\{(.*?)\}\s*;', text, flags=re.S):
        enums[name] = {k: int(v) for k, v in re.findall(r'(\w+)\s*=\s*(-?\d+)', body)}
    return signatures, restypes, structs, enums


with open(HEADER_PATH) as _f:
    SIGNATURES, RESTYPES, STRUCTS, ENUMS = read_header(_f.read())


class WgradJob(ctypes.Structure):
    _fields_ = STRUCTS['stj_wgrad_job']


class AgentWeights(ctypes.Structure):
    _fields_ = STRUCTS['stj_agent_weights']


class AgentEncArgs(ctypes.Structure):
    _fields_ = STRUCTS['stj_agent_enc_args']


class AgentIntArgs(ctypes.Structure):
    _fields_ = STRUCTS['stj_agent_int_args']


class FgOffArgs(ctypes.Structure):
    _fields_ = STRUCTS['stj_fgoff_args']


_lib = None


def lib():
    """Load (once) and return the C-ABI library.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise StjError(f'{LIB_PATH} not found: build it with `python -m strajnet_amd.build` '
                           '(hipcc --offload-arch=gfx950).  There is no CPU / eager fallback.')
        L = ctypes.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError here == header / library mismatch
            fn.argtypes = args
            fn.restype = RESTYPES[name]
        L.stj_last_error.argtypes = []
        L.stj_last_error.restype = ctypes.c_char_p
        _lib = L
    return _lib


def call(name, *args):
    L = lib()
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise StjError(f'{name} failed ({rc}): {L.stj_last_error().decode()}')
