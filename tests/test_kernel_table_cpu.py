"""
The table of kernels launched with dynamic LDS (csrc/swiftly_launch.h), asked without a GPU through
``swiftly_hip_kernel_table``.  Every such launch registers its (kernel, LDS bytes) pair while the library is loaded, and
``swiftly_hip_create`` sets the per-device attribute of every entry; this is what a machine without a device can see of it.
"""
import ctypes


def test_kernel_table_is_shared_and_needs_the_opt_in():
    from ska_sdp_exec_swiftly_amd import _lib

    count, max_lds = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert _lib.load().swiftly_hip_kernel_table(ctypes.byref(count), ctypes.byref(max_lds)) == 0
    print(f"kernel table: {count.value} instances, largest LDS {max_lds.value} bytes")
    # the entry point sits in a translation unit that launches nothing with LDS: a table kept per translation unit would be empty
    assert count.value > 0
    # above 64 KiB the opt-in is needed at all (the 65536-point band geometry alone asks for about 132 KB); a CU has 160 KiB
    assert 64 * 1024 < max_lds.value <= 160 * 1024
