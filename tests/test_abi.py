"""The C-ABI shared library loads without a GPU and exports every symbol include/p2pb_hip.h declares."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "p2pb_hip.h")


def header_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(p2pb_\w+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from p2p_bridge_amd import _lib, build

    build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/p2pb_hip.h but not exported"
    assert sorted(_lib.SYMBOLS) == syms
    assert _lib.lib().p2pb_target_arch() == b"gfx950"


def test_binding_types_every_declared_symbol_from_the_header():
    """_lib parses the header into the table lib() types the library with: the same names as the independent regex above, and
    every one of them carries its restype and argtypes on the loaded library"""
    from p2p_bridge_amd import _lib, build

    build.build()
    syms = header_symbols()
    table, version = _lib.parse_header(open(HDR).read())
    assert sorted(table) == syms == sorted(_lib.SIGNATURES) and version == _lib.ABI_VERSION
    lib = _lib.lib()
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and list(fn.argtypes) == table[s][1] and fn.restype is table[s][0], s


def test_binding_types_match_hand_written_anchors():
    """signatures written out here from the header's text, not derived through the parser"""
    from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_longlong, c_size_t, c_void_p

    from p2p_bridge_amd import _lib

    lib = _lib.lib()
    assert lib.p2pb_knn_points_ws_bytes.restype is c_size_t and list(lib.p2pb_knn_points_ws_bytes.argtypes) == [c_int] * 3
    assert lib.p2pb_target_arch.restype is c_char_p and list(lib.p2pb_target_arch.argtypes) == []
    a = lib.p2pb_linear_rows.argtypes
    assert len(a) == 11 and all(a[i] is c_long for i in (4, 6, 9)) and all(a[i] is c_void_p for i in (3, 5, 7, 8, 10))
    assert all(a[i] is c_int for i in (0, 1, 2)) and lib.p2pb_linear_rows.restype is c_int
    assert lib.p2pb_voxel_coords.argtypes[4] is c_float
    assert all(lib.p2pb_optim_clip_adam_step.argtypes[i] is c_double for i in range(5, 10))
    assert lib.p2pb_optim_clip_adam_step.argtypes[4] is c_void_p and lib.p2pb_optim_clip_adam_step.argtypes[10] is c_int
    assert lib.p2pb_row_max_forward.argtypes[0] is c_long
    assert lib.p2pb_pairwise_emd.argtypes[8] is c_size_t
    assert lib.p2pb_debug_pointwise_form.argtypes[3] is c_void_p
    assert lib.p2pb_scan_segment_mean.argtypes[0] is c_longlong


def test_binding_refuses_a_wrong_argument_count():
    """ctypes itself passes surplus arguments of a cdecl function on silently: call() and ask() compare the count first
    (host-state entry points only: nothing is launched)"""
    from p2p_bridge_amd import _lib

    base = _lib.ask("p2pb_get_split_terms")
    with pytest.raises(_lib.P2PBError, match=r"p2pb_set_split_terms_thread takes 1 .* called with 2"):
        _lib.call("p2pb_set_split_terms_thread", 0, 0)
    with pytest.raises(_lib.P2PBError, match=r"p2pb_set_split_terms_thread takes 1 .* called with 0"):
        _lib.call("p2pb_set_split_terms_thread")
    with pytest.raises(_lib.P2PBError, match=r"p2pb_conv3d_k3_stats_floats takes 3 .* called with 2"):
        _lib.ask("p2pb_conv3d_k3_stats_floats", 1, 8)
    with pytest.raises(_lib.P2PBError, match=r"p2pb_conv3d_k3_stats_floats takes 3 .* called with 4"):
        _lib.ask("p2pb_conv3d_k3_stats_floats", 1, 8, 8, 8)
    assert _lib.call("p2pb_set_split_terms_thread", 0) is None
    assert _lib.ask("p2pb_conv3d_k3_stats_floats", 1, 8, 8) > 0
    assert _lib.ask("p2pb_get_split_terms") == base


def test_binding_refuses_a_wrong_argument_type():
    """a float for an int parameter, a C int for a long long one (host-only entry points; the conversion fails before the call)"""
    from p2p_bridge_amd import _lib

    with pytest.raises(ctypes.ArgumentError):
        _lib.ask("p2pb_conv3d_k3_stats_floats", 1.5, 8, 8)
    with pytest.raises(ctypes.ArgumentError):
        _lib.call("p2pb_set_split_terms_thread", 1.5)
    with pytest.raises(ctypes.ArgumentError):
        _lib.ask("p2pb_room_fps_jobs_ws_bytes", ctypes.c_int(7))
    assert _lib.ask("p2pb_room_fps_jobs_ws_bytes", 7) == _lib.ask("p2pb_room_fps_jobs_ws_bytes", ctypes.c_longlong(7))
    assert _lib.ask("p2pb_room_fps_jobs_ws_bytes", 2 ** 33) == 16 * 2 ** 33  # (neither narrowed to a C int on the way in nor out)


def test_parser_refuses_a_header_it_cannot_type():
    from p2p_bridge_amd import _lib

    text = open(HDR).read()
    good = "int p2pb_voxel_coords(int b, int n, int r, int normalize, float eps,"
    assert text.count(good) == 1
    for bad in (good.replace("float eps", "half eps"), good.replace("float eps", "float"), good.replace("int p2pb", "status_t p2pb"),
                good.replace("int r,", "int r[3],")):
        with pytest.raises(_lib.P2PBError, match="p2pb_voxel_coords"):
            _lib.parse_header(text.replace(good, bad))
    with pytest.raises(_lib.P2PBError, match="p2pb_x"):
        _lib.parse_header(text.replace(good, "#define P2PB_X(a) p2pb_x(a)\n" + good) + "\nstatic inline int f(void) { return p2pb_x(1); }\n")
    with pytest.raises(_lib.P2PBError, match="p2pb_voxel_coords"):
        _lib.parse_header(text + "\nint p2pb_voxel_coords(int b);\n")  # declared twice
    with pytest.raises(_lib.P2PBError, match="P2PB_ABI_VERSION"):
        _lib.parse_header(text.replace("#define P2PB_ABI_VERSION", "#define P2PB_ABI_VERSION_"))


def test_library_contains_gfx950_code_object():
    from p2p_bridge_amd import _lib

    out = subprocess.run(["strings", "-n", "6", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_no_kernel_issues_ds_write_b96():
    """Round 4's cross-stream corruption (docs/history/DESIGN_round5.md, section 3.5) sat in a kernel whose LDS staging the compiler had merged into
    ds_write_b96 + ds_write2_b32; the mechanism is unexplained (barrier and s_waitcnt were in order in the ISA), so the invariant
    that protects the library is enforced here: the disassembly of every translation unit of libp2pb_hip.so holds no 12-byte LDS
    store. (tests/test_concurrency_gpu.py is the dynamic half of the net.)"""
    import glob
    import tempfile

    from p2p_bridge_amd import build

    build.build()
    llvm = "/opt/rocm/lib/llvm/bin"
    objs = sorted(glob.glob(os.path.join(build.OBJ, "*.o")))
    assert len(objs) >= 16
    seen_b128 = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            fat, co = os.path.join(tmp, "x.fat"), os.path.join(tmp, "x.co")
            subprocess.run([f"{llvm}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", o], check=True)
            subprocess.run([f"{llvm}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
            isa = subprocess.run([f"{llvm}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
            assert "s_endpgm" in isa, o
            seen_b128 += isa.count("ds_write_b128")
            for bad in ("ds_write_b96", "ds_store_b96"):
                assert bad not in isa, (bad, os.path.basename(o))
    assert seen_b128 > 100  # (the grep sees LDS stores at all)


def test_no_cpu_fallback():
    """product ops refuse CPU tensors (the oracle is never a fallback)."""
    import torch

    from p2p_bridge_amd import pointnet2_batch_cuda as ext

    with pytest.raises(RuntimeError):
        ext.furthest_point_sampling_forward(torch.zeros(1, 3, 16), 4)
    with pytest.raises(RuntimeError):
        ext.avg_voxelize_forward(torch.zeros(1, 2, 16), torch.zeros(1, 3, 16, dtype=torch.int32), 4)


def test_product_never_imports_oracle():
    import glob

    for f in glob.glob(os.path.join(ROOT, "p2p_bridge_amd", "**", "*.py"), recursive=True):
        src = open(f).read()
        assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f
        assert "cpu_ops" not in src, f


def test_split_terms_thread_override_is_per_thread():
    """p2pb_set_split_terms_thread (fused.split_math): a temporary arithmetic switch on one thread is invisible to the
    others; the process-wide setter still reaches every thread without an override (no GPU needed: host state only)"""
    import threading

    from p2p_bridge_amd import _lib

    lib = _lib.lib()
    base = lib.p2pb_get_split_terms()
    seen = {}

    def worker():
        assert lib.p2pb_set_split_terms_thread(6) == 0
        seen["inside"] = lib.p2pb_get_split_terms()
        ev1.set()
        ev2.wait(5)
        assert lib.p2pb_set_split_terms_thread(0) == 0
        seen["cleared"] = lib.p2pb_get_split_terms()

    ev1, ev2 = threading.Event(), threading.Event()
    t = threading.Thread(target=worker)
    t.start()
    ev1.wait(5)
    seen["other_thread"] = lib.p2pb_get_split_terms()
    ev2.set()
    t.join()
    assert seen == {"inside": 6, "other_thread": base, "cleared": base}
    assert lib.p2pb_set_split_terms_thread(5) != 0  # not an arithmetic


def test_abi_version_matches_header_and_binding():
    """p2pb_version() used to return 1 through every ABI change. Header macro == library == binding, and the loader
    refuses a library of another version (a stale .so behind P2PB_LIB_PATH) with a message instead of failing late."""
    from p2p_bridge_amd import _lib, build

    build.build()
    macro = int(re.search(r"#define\s+P2PB_ABI_VERSION\s+(\d+)", open(HDR).read()).group(1))
    assert macro == _lib.ABI_VERSION
    assert ctypes.CDLL(_lib.LIB_PATH).p2pb_version() == macro
    code = ("import p2p_bridge_amd._lib as L\n"
            "L.ABI_VERSION += 1\n"
            "try:\n    L.lib()\nexcept L.P2PBError as e:\n    assert 'ABI version' in str(e), e\n    print('refused')\n")
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "refused" in r.stdout, r.stderr[-2000:]


def test_experiment_switch_parsers_agree_and_legacy_names_warn():
    """the C parser (csrc/abi.hip p2pb_experiment_long) reads P2PB_EXPERIMENT like the Python one
    (p2p_bridge_amd/_experiment.py; the C function is internal to the library, reached by its mangled name): case-insensitive keys, blanks around key, '=' and value; and a pre-round-5 switch name
    in the environment (silently ignored since) raises a RuntimeWarning naming its replacement."""
    code = r'''
import ctypes, os, warnings
os.environ["P2PB_EXPERIMENT"] = " Pw_Pp = 0 ;conv_wide_min=77; FPS_MID =9;x=1"
from p2p_bridge_amd import _lib, _experiment
so = ctypes.CDLL(_lib.LIB_PATH)
f = getattr(so, "_Z20p2pb_experiment_longPKcl"); f.restype = ctypes.c_long; f.argtypes = [ctypes.c_char_p, ctypes.c_long]
for key, dflt in (("pw_pp", 1), ("conv_wide_min", 256), ("fps_mid", 512), ("absent", 5), ("pw", 3), ("x", 0)):
    assert f(key.encode(), dflt) == _experiment.get_int(key, dflt), (key, f(key.encode(), dflt), _experiment.get_int(key, dflt))
assert f(b"pw_pp", 1) == 0 and f(b"fps_mid", 512) == 9 and f(b"pw", 3) == 3
os.environ["P2PB_FPS_BIG"] = "coop"
with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    _experiment.get("fps_big")
    _experiment.get("fps_big")
assert len(w) == 1 and "fps_big" in str(w[0].message) and issubclass(w[0].category, RuntimeWarning), [str(x.message) for x in w]
print("ok")
'''
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr[-2000:]
