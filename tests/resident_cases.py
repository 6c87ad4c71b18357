"""What the CPU and GPU tests of the resident store share: the fp32 bit patterns the conversion is held on, and the host library's
answer to them (freud_f32_to_bf16_portable of libfreud_host.so: the rule the loader delivers by)."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def convert_table() -> np.ndarray:
    """uint32: every bf16 high half crossed with six low halves (ties, just below, just above, the ends); the 64 fp32 neighbours on
    each side of -1.0 and -1.0 itself; +-0, denormals, +-inf and NaN payloads."""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    lows = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    grid = (hi[:, None] | lows[None, :]).reshape(-1)
    near = (0xBF800000 + np.arange(-64, 65, dtype=np.int64)).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x00400000,
                        0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800001, 0xFF800001, 0x7F80FFFF, 0x7FBFFFFF, 0x7FC00000,
                        0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FFF8000, 0x3F800000, 0xBF800000, 0xBF7FFFFF, 0xBF800001, 0xBF7F8000,
                        0xBF808000, 0xBF7F7FFF, 0xBF80FFFF], dtype=np.uint32)
    out = np.concatenate([grid, near, special])
    out.setflags(write=False)
    return out


def host_convert(u32: np.ndarray) -> np.ndarray:
    """bf16 bit patterns (uint16) of the fp32 bit patterns u32, by libfreud_host.so's portable loop."""
    from freud_amd.loader import _host_lib
    src = np.ascontiguousarray(u32, dtype=np.uint32)
    dst = np.empty(src.shape, dtype=np.uint16)
    _host_lib().freud_f32_to_bf16_portable(src.ctypes.data, dst.ctypes.data, src.size)
    return dst


@functools.lru_cache(maxsize=None)
def convert_expected() -> np.ndarray:
    out = host_convert(convert_table())
    out.setflags(write=False)
    return out
