"""ctypes binding of the C-ABI library ``libcmx_hip.so``.

The argument/return types are derived by parsing ``include/cmx_hip.h`` (shipped inside
the package as ``cmx_hip.h``), so the header is the single source of truth for the ABI.
``include/cmx_ohem.h`` (part 2 of the same library's ABI: the OHEM loss and its select) is parsed the
same way into a table of its own, ``OHEM_SIGNATURES``; its entry points are called like any other.
``include/cmx_easpp.h`` (part 3: the eASPP neck of the ``mit_b*_w_ef_aspp`` backbones) likewise, into
``EASPP_SIGNATURES``.  ``include/cmx_fcn.h`` (part 4: the fused upsample + loss at the scales of an FCN head)
likewise, into ``FCN_SIGNATURES``.  ``include/cmx_deeplab.h`` (part 5: the DeepLabV3+ head's wide dilated convolution and
align-corners upsample + concat) likewise, into ``DEEPLAB_SIGNATURES``.  ``include/cmx_mlp.h`` (part 6: the Mix-FFN of stages
1-2 with its Linears inside the depthwise kernels) likewise, into ``MLP_SIGNATURES``.  ``include/cmx_uper.h`` (part 7: the
UPerNet head's pyramid pooling, multi-source upsample + concat, upsample + add and the weight flip of the im2col-free
input gradient) likewise, into ``UPER_SIGNATURES``.

``call`` / ``try_call`` / ``query`` / ``refusable`` take an entry point's name and its arguments in
header order; ``marshal`` converts them by the kind the header declares for each parameter:
 * pointer (any ``*`` but ``const char*``): a ``torch.Tensor`` (its ``data_ptr()``: a view passes its
   own address, nothing is copied), ``None`` (NULL) or an integer address, passed through unchanged;
 * stream (``hipStream_t``, always last): an integer handle; left out, ``stream()`` is appended;
 * scalar (the rest): a Python number (``bool`` becomes ``int``) or ``bytes``, never a tensor.
Any other argument count is a ``TypeError`` (ctypes alone accepts surplus arguments silently).

The library is loaded AFTER ``import torch`` so that its ``libamdhip64.so.7`` dependency
resolves (by SONAME) to the HIP runtime torch already loaded: kernels then run on torch's
streams and are captured by torch's HIP graphs.  There is no fallback: if the library is
missing or fails to load, importing the product raises.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# CMX_LIB_VARIANT=name loads libcmx_hip_<name>.so (an A/B build of the same sources with other
# compile-time options, csrc/Makefile VARIANT=); default: libcmx_hip.so
_VARIANT = os.environ.get("CMX_LIB_VARIANT", "")
LIB_PATH = os.path.join(_HERE, f"libcmx_hip_{_VARIANT}.so" if _VARIANT else "libcmx_hip.so")
HEADER_PATHS = [os.path.join(_HERE, "..", "include", "cmx_hip.h"), os.path.join(_HERE, "cmx_hip.h")]
OHEM_HEADER_PATHS = [os.path.join(_HERE, "..", "include", "cmx_ohem.h"), os.path.join(_HERE, "cmx_ohem.h")]
EASPP_HEADER_PATHS = [os.path.join(_HERE, "..", "include", "cmx_easpp.h"), os.path.join(_HERE, "cmx_easpp.h")]
FCN_HEADER_PATHS = [os.path.join(_HERE, "..", "include", "cmx_fcn.h"), os.path.join(_HERE, "cmx_fcn.h")]
DEEPLAB_HEADER_PATHS = [os.path.join(_HERE, "..", "include", "cmx_deeplab.h"), os.path.join(_HERE, "cmx_deeplab.h")]
MLP_HEADER_PATHS = [os.path.join(_HERE, "..", "include", "cmx_mlp.h"), os.path.join(_HERE, "cmx_mlp.h")]
UPER_HEADER_PATHS = [os.path.join(_HERE, "..", "include", "cmx_uper.h"), os.path.join(_HERE, "cmx_uper.h")]


class CMXError(RuntimeError):
    pass


# cmx_status codes (csrc/cmx_common.h)
CMX_OK, CMX_ERR_SHAPE, CMX_ERR_DTYPE, CMX_ERR_LAUNCH, CMX_ERR_ARG = 0, -1, -2, -3, -4


def _ctype(decl: str):
    decl = decl.strip()
    if "*" in decl:
        if decl.startswith("const char") and decl.count("*") == 1 and not decl.split("*")[1].strip():
            return ctypes.c_char_p
        return ctypes.c_void_p
    base = decl.rsplit(" ", 1)[0] if " " in decl else decl
    base = base.replace("const", "").strip()
    return {"int": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
            "size_t": ctypes.c_size_t, "double": ctypes.c_double, "hipStream_t": ctypes.c_void_p, "void": None}[base]


POINTER, STREAM, SCALAR = "pointer", "stream", "scalar"


def _kind(decl: str) -> str:
    if "*" in decl:
        return SCALAR if decl.strip().startswith("const char") else POINTER     # a C string: bytes
    return STREAM if "hipStream_t" in decl.split() else SCALAR


class Signature(tuple):
    """(restype, [argtypes]) of one declaration; ``kinds`` holds POINTER / STREAM / SCALAR per parameter."""
    kinds: tuple = ()


def _header(path: str | None) -> str:
    return open(path or next(p for p in HEADER_PATHS if os.path.exists(p))).read()


def parse_header(path: str | None = None):
    """Return {name: Signature (restype, [argtypes]), .kinds} for every declaration in the header at
    ``path`` (default: cmx_hip.h)."""
    text = re.sub(r"/\*.*?\*/", "", _header(path), flags=re.S)
    out = {}
    for m in re.finditer(r"^\s*([A-Za-z_][\w\s\*]*?)\b(cmx_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        rt = ctypes.c_char_p if ret.strip() == "const char*" else _ctype(ret.strip() + " r")
        decls = [] if args in ("", "void") else args.split(",")
        out[name] = Signature((rt, [_ctype(a) for a in decls]))
        out[name].kinds = tuple(_kind(a) for a in decls)
    return out


def header_abi_version(path: str | None = None) -> int:
    """The CMX_ABI_VERSION the header defines (the revision the bindings below are parsed from)."""
    m = re.search(r"^#define\s+CMX_ABI_VERSION\s+(\d+)", _header(path), re.M)
    if m is None:
        raise CMXError(f"{path or 'cmx_hip.h'} defines no CMX_ABI_VERSION")
    return int(m.group(1))


def _load():
    if not os.path.exists(LIB_PATH):
        raise CMXError(f"libcmx_hip.so not found at {LIB_PATH}; run __graft_entry__.build() "
                       "(or `make -C rgbx_semantic_segmentation_amd/csrc`).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.cmx_abi_version.restype = ctypes.c_int32
    lib.cmx_abi_version.argtypes = []
    want, have = header_abi_version(), int(lib.cmx_abi_version())
    if have != want:
        raise CMXError(f"{LIB_PATH} was built for C-ABI revision {have}, the header declares {want}: "
                       "rebuild it (`make -C rgbx_semantic_segmentation_amd/csrc`)")
    sigs = parse_header()
    ohem = parse_header(next(p for p in OHEM_HEADER_PATHS if os.path.exists(p)))
    easpp = parse_header(next(p for p in EASPP_HEADER_PATHS if os.path.exists(p)))
    fcn = parse_header(next(p for p in FCN_HEADER_PATHS if os.path.exists(p)))
    deeplab = parse_header(next(p for p in DEEPLAB_HEADER_PATHS if os.path.exists(p)))
    mlp = parse_header(next(p for p in MLP_HEADER_PATHS if os.path.exists(p)))
    uper = parse_header(next(p for p in UPER_HEADER_PATHS if os.path.exists(p)))
    for table in (sigs, ohem, easpp, fcn, deeplab, mlp, uper):
        for name, (rt, argt) in table.items():
            fn = getattr(lib, name)
            fn.argtypes = argt
            fn.restype = rt
            assert STREAM not in table[name].kinds[:-1], f"{name}: hipStream_t must be the last parameter"
    return lib, sigs, ohem, easpp, fcn, deeplab, mlp, uper


(LIB, SIGNATURES, OHEM_SIGNATURES, EASPP_SIGNATURES, FCN_SIGNATURES, DEEPLAB_SIGNATURES, MLP_SIGNATURES,
 UPER_SIGNATURES) = _load()


def last_error() -> str:
    return LIB.cmx_last_error().decode()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _pointer_arg(a):
    return a.data_ptr() if isinstance(a, torch.Tensor) else a


def _scalar_arg(a):
    if isinstance(a, torch.Tensor):
        raise TypeError("a tensor was passed where the header declares a scalar")
    return int(a) if a is True or a is False else a


# per entry point, built once: (the C function, one converter per parameter, takes a trailing stream)
_BOUND = {name: (getattr(LIB, name), tuple(_pointer_arg if k == POINTER else _scalar_arg for k in sig.kinds),
                 sig.kinds[-1:] == (STREAM,))
          for name, sig in {**SIGNATURES, **OHEM_SIGNATURES, **EASPP_SIGNATURES, **FCN_SIGNATURES,
                            **DEEPLAB_SIGNATURES, **MLP_SIGNATURES, **UPER_SIGNATURES}.items()}


def marshal(name: str, args: tuple) -> tuple:
    """The argument tuple ctypes is given for ``args`` of entry point ``name`` (module docstring)."""
    _, convs, takes_stream = _BOUND[name]
    if len(args) != len(convs):
        if not (takes_stream and len(args) == len(convs) - 1):
            raise TypeError(f"{name} takes {len(convs)} arguments, {len(args)} given")
        args = (*args, stream())
    return tuple([c(a) for c, a in zip(convs, args)])


# measurement hook (roofline.measure_gemm_family): observer(name, fn, args) runs right after a
# successful call with the marshalled arguments (fn(*args) repeats the launch), while the caller
# still holds every buffer they point to
observer = None


def try_call(name: str, *args) -> int:
    """Invoke an int-returning entry point and return its status (the caller decides what a
    refusal means); the measurement observer sees it only when it succeeded."""
    fn = _BOUND[name][0]
    args = marshal(name, args)
    st = int(fn(*args))
    if st == 0 and observer is not None:
        observer(name, fn, args)
    return st


def call(name: str, *args) -> None:
    """Invoke an int-returning entry point; raise CMXError on a negative status."""
    refusable(name, (), *args)


REFUSED = object()


def refusable(name: str, refusals: tuple, *args):
    """``call``, except that a status among ``refusals`` (the entry point declines this problem:
    CMX_ERR_ARG / CMX_ERR_SHAPE) returns REFUSED for the caller to take another path."""
    st = try_call(name, *args)
    if st in refusals:
        return REFUSED
    if st != 0:
        raise CMXError(f"{name} failed ({st}): {last_error()}")


def query(name: str, *args) -> int:
    return int(_BOUND[name][0](*marshal(name, args)))


# the dtype codes of the C-ABI (cmx_dtype)
DTYPE_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def dtype_code(t: torch.Tensor) -> int:
    if t.dtype not in DTYPE_CODES:
        raise CMXError(f"unsupported dtype {t.dtype}")
    return DTYPE_CODES[t.dtype]
