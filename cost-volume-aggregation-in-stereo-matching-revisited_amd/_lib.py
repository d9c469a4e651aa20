"""ctypes binding of include/dca_hip.h, READ from the header at import: SIGNATURES (every `int|long dca_*(...)`
declaration) and CONSTANTS (every integer `#define DCA_*`).  Adding an entry point is: declare it in dca_hip.h, define it
in a .hip file that sees the header, call it.  There is NO fallback: if the header or libdca_hip.so is missing, or the
library does not export every symbol the header declares, importing the ops raises."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdca_hip.so")
HEADER = os.path.join(HERE, "..", "include", "dca_hip.h")

_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
          "hipStream_t": ctypes.c_void_p}


def _ctype(fn, param):
    """ctypes type of one parameter declaration `type name`; a type outside _TYPES is not guessed at"""
    if "*" in param:
        return ctypes.c_void_p
    words = [w for w in param.split()[:-1] if w != "const"]
    if len(words) != 1 or words[0] not in _TYPES:
        raise RuntimeError(f"include/dca_hip.h: {fn}: parameter `{param.strip()}` has a type the binding does not know")
    return _TYPES[words[0]]


def parse_header(text):
    """header text -> (SIGNATURES: name -> (restype, [argtypes]), CONSTANTS: DCA_* -> int)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    sigs = {}
    for ret, fn, params in re.findall(r"^(int|long) (dca_\w+)\s*\(([^;]*)\);", text, flags=re.M):
        params = [] if params.strip() == "void" else params.split(",")
        sigs[fn] = (_TYPES[ret], [_ctype(fn, p) for p in params])
    if not sigs:
        raise RuntimeError("include/dca_hip.h: no `int|long dca_*(...);` declaration found")
    consts = {k: int(v, 0) for k, v in re.findall(r"^#define (DCA_\w+) (-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, flags=re.M)}
    return sigs, consts


if not os.path.exists(HEADER):
    raise RuntimeError(f"{HEADER} not found: the binding is read from it")
with open(HEADER) as _f:
    SIGNATURES, CONSTANTS = parse_header(_f.read())
ABI_VERSION = CONSTANTS["DCA_ABI_VERSION"]

_lib = None


def load():
    """Loads the HIP library and binds every C-ABI symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the DCANet hot path has no CPU/PyTorch fallback. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950).")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing -> loud
        fn.restype, fn.argtypes = res, args
    got = lib.dca_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} was built from another version of include/dca_hip.h (ABI {got}, this package "
                           f"binds ABI {ABI_VERSION}): rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`")
    _lib = lib
    return lib
