"""What the ABI tests share, each thing written once: where the LLVM tools are, the code a create call answers without a
context, the library's last error text, the scratch bytes of the library's gfx950 kernels, and the agreement of a side
header with its binding module and the library's export table."""
import ctypes as C
import re
import shutil
import subprocess

from libsdr_amd import abi, nodes

LLVM = "/opt/rocm/lib/llvm/bin/"


def no_ctx_code():
    """What a create call with valid arguments and a NULL context answers: there is a device or there is none."""
    return abi.E_NODEVICE if nodes.device_count() == 0 else abi.E_INVALID


def last_error():
    return abi.lib().sdrhip_last_error().decode()


def code_objects(tmp_path):
    """The library's gfx950 code objects, extracted into tmp_path."""
    so = shutil.copy(abi.SO_PATH, tmp_path / "lib.so")
    subprocess.run([LLVM + "llvm-objdump", "--offloading", str(so)], capture_output=True, text=True, check=True, cwd=tmp_path)
    return sorted(tmp_path.glob("lib.so.*gfx950"))


def kernels(objs):
    """(code object, mangled kernel name, private_segment_fixed_size) of every kernel in the code objects."""
    for o in objs:
        notes = subprocess.run([LLVM + "llvm-readelf", "--notes", str(o)], capture_output=True, text=True).stdout
        for name, scratch in re.findall(r"\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)", notes):
            yield o, name, int(scratch)


def kernel_scratch(tmp_path, pattern):
    """{kernel: scratch bytes} of every gfx950 kernel whose mangled name `pattern` finds: keyed by the pattern's group (the
    tuple of its groups where it has several, the whole mangled name where it has none)."""
    seen = {}
    for _, name, scratch in kernels(code_objects(tmp_path)):
        m = re.search(pattern, name)
        if m:
            seen[name if not m.re.groups else m.group(1) if m.re.groups == 1 else m.groups()] = scratch
    return seen


def assert_header_binding(module, names, export_regex):
    """The header of the binding module declares exactly `names`, the module has a prototype for each, libsdrhip.so exports
    each — and nothing else that export_regex finds — and module.lib() is abi.lib() with the prototypes applied."""
    declared = module.header_functions()
    assert declared == sorted(names)
    assert sorted(module.SIGNATURES) == declared
    fresh = C.CDLL(abi.SO_PATH)   # (looked up by name in the library's own export table, not through the binding)
    for f in declared:
        assert C.cast(getattr(fresh, f), C.c_void_p).value, f
    L = module.lib()
    assert L is abi.lib()
    for f, (res, args) in module.SIGNATURES.items():
        fn = getattr(L, f)
        assert fn.restype is res and list(fn.argtypes) == args, f
    syms = subprocess.run([LLVM + "llvm-readelf", "--dyn-syms", "-W", abi.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(export_regex, syms))) == declared
