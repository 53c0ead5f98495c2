"""ctypes view of include/sdso_abi.h, the one door into libsdso_hip.so for everything that is not C++.  This module is the public name;
the parts live next to it, by concern:

  abi_types    the structures and constants of the header (tests/test_abi_layout_cpu.py holds them to the compiled header)
  abi_marshal  numpy -> pointers: ptr, bind, the unchecked fp / dp / ip / bp, the make_* builders
  abi_lib      SIGNATURES (one entry per exported function, = EXPORTED_SYMBOLS), declare, load, LIB_PATH
  abi_context  SdsoError, Shared, Pool, Context

There is no CPU fallback: load() raises if the HIP library has not been built, and Context() raises if no MI355X/HIP device is usable.
"""
from .abi_types import *      # noqa: F401,F403
from .abi_marshal import *    # noqa: F401,F403
from .abi_lib import LIB_PATH, SIGNATURES, EXPORTED_SYMBOLS, declare, load   # noqa: F401
from .abi_context import SdsoError, Shared, Pool, Context   # noqa: F401
