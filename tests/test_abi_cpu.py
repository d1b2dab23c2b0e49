"""The C-ABI library loads and exports every symbol include/*.h declares; without a GPU every
compute entry point fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quilt_amd import native


def _declared_functions():
    import glob
    names = set()
    for header in glob.glob(os.path.join(os.path.dirname(native.HEADER), "*.h")):   # quilt_amd.h, quilt_amd_io.h
        text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        names |= set(re.findall(r"\b(qa_[a-zA-Z0-9_]+)\s*\(", text))
    return sorted(names)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def test_every_declared_symbol_is_exported(lib):
    names = _declared_functions()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/*.h but not exported"
    assert lib.qa_abi_version() == 5


def test_no_cpu_fallback_without_a_device(lib):
    if lib.qa_device_count() > 0:
        pytest.skip("a gfx950 device is present")
    h = C.c_void_p()
    d = native.PanelDesc()
    assert lib.qa_panel_create(C.byref(d), C.byref(h)) == native.QA_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.qa_last_error()
    gl = np.ones((2, 4))
    assert lib.qa_Rcpp_haploid_dosage_versus_refs(None, native.ptr(gl), None, None, None, None, None, None, None,
                                                  None, None, None, None, C.c_int64(0)) == native.QA_ERR_NO_DEVICE
    assert lib.qa_gibbs_batch(None, None, 1, None, None, None, None, None, None, None, None, None, None, None, None,
                              None, None, None, None, None, None) == native.QA_ERR_NO_DEVICE
    with pytest.raises(native.QuiltAmdError):
        native.check(lib.qa_set_device(0))


def _header_prototypes():
    """{name: parameter count} of include/*.h, by a scan of its own (not native.prototypes): the text between a declared name's
    parentheses, split at the commas."""
    import glob
    counts = {}
    for header in glob.glob(os.path.join(os.path.dirname(native.HEADER), "*.h")):
        text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        for name, params in re.findall(r"\b(qa_[a-zA-Z0-9_]+)\s*\(([^()]*)\)\s*;", text):
            counts[name] = 0 if params.strip() == "void" else params.count(",") + 1
    return counts


def test_every_declared_function_has_its_prototype(lib):
    counts = _header_prototypes()
    names = _declared_functions()
    assert set(counts) == set(names)
    for n in names:
        f = getattr(lib, n)
        assert f.argtypes is not None, f"{n} has no argtypes"
        assert len(f.argtypes) == counts[n], f"{n}: {len(f.argtypes)} argtypes, {counts[n]} parameters in the header"
    restype = lambda n: getattr(lib, n).restype
    assert (restype("qa_host_alloc"), getattr(lib, "qa_host_alloc").argtypes) == (C.c_void_p, [C.c_size_t])
    assert restype("qa_mspbwt_create") is C.c_void_p
    for n in ("qa_mspbwt_bytes", "qa_mspbwt_find_good_matches", "qa_sample_reads_n_bases", "qa_sample_reads_names_bytes"):
        assert restype(n) is C.c_int64, n
    for n in ("qa_last_error", "qa_profile_name", "qa_vcf_missing_entry"):
        assert restype(n) is C.c_char_p, n
    text = "".join(open(os.path.join(os.path.dirname(native.HEADER), h)).read() for h in ("quilt_amd.h", "quilt_amd_io.h"))
    void_functions = re.findall(r"^void\s+(qa_\w+)\s*\(", text, flags=re.M)
    assert len(void_functions) >= 8
    for n in names:
        assert (restype(n) is None) == (n in void_functions), n


def test_the_prototype_parser_reads_the_shapes_the_headers_use():
    text = """
    /* a comment with qa_not_a_function(int x); in it */
    #include <stdint.h>
    #ifdef __cplusplus
    extern "C" {
    #endif
    typedef struct qa_thing qa_thing_t;   // opaque
    typedef struct { int32_t a; void (*cb)(void *ctx, int32_t x); double v[4]; } qa_opts_t;
    typedef int (*qa_visit_fn)(void *handle, int32_t n,
                               double *out);
    int qa_three_lines(qa_thing_t *t, int32_t n,
                       const double *x, int64_t cap,
                       size_t bytes, double q);
    int qa_nothing(void);
    int qa_array(int32_t device, double out[7]);
    int qa_handles(qa_thing_t *const *things, int n, const qa_opts_t *opts);
    const char *qa_text(void);
    qa_thing_t *qa_make(const char *path);
    void *qa_raw(size_t bytes);
    void qa_drop(qa_thing_t *t);
    int64_t qa_count(const qa_thing_t *t);
    int qa_visit(qa_visit_fn visit, void *const *handles);
    #ifdef __cplusplus
    }
    #endif
    """
    P, I32, I64, D = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    assert native.prototypes(text) == {
        "qa_three_lines": (C.c_int, [P, I32, P, I64, C.c_size_t, D]), "qa_nothing": (C.c_int, []), "qa_array": (C.c_int, [I32, P]),
        "qa_handles": (C.c_int, [P, C.c_int, P]), "qa_text": (C.c_char_p, []), "qa_make": (P, [P]), "qa_raw": (P, [C.c_size_t]),
        "qa_drop": (None, [P]), "qa_count": (I64, [P]), "qa_visit": (C.c_int, [P, P]),
    }
    for bad in ("int qa_unknown_scalar(int32_t n, float x);", "unsigned qa_unknown_return(void);", "int qa_by_value(qa_opts_t opts);"):
        with pytest.raises(TypeError, match=bad.split("(")[0].split()[-1]):
            native.prototypes(bad)
    with pytest.raises(TypeError):
        native.prototypes("int qa_fine(void); static const int x = 3;")   # (text that is no declaration does not pass silently)


def test_a_wrong_argument_raises_instead_of_passing(lib):
    ms, n, b = C.c_double(), C.c_int64(), C.c_double()
    with pytest.raises(C.ArgumentError):
        lib.qa_profile_get(0.5, C.byref(ms), C.byref(n), C.byref(b))
    gl = np.ones((2, 4))
    with pytest.raises(C.ArgumentError):   # (best_cap is an int64_t: a 32-bit wrapper left the register's upper half undefined)
        lib.qa_Rcpp_haploid_dosage_versus_refs(None, native.ptr(gl), None, None, None, None, None, None, None, None, None, None,
                                               None, C.c_int32(0))
    with pytest.raises(C.ArgumentError):
        lib.qa_host_alloc(C.c_int64(64))


def test_prototypes_are_declared_in_one_place():
    """No file of the package, tests/, scripts/ or the build entry assigns restype / argtypes on a qa_* function: quilt_amd/native.py
    takes every prototype from the headers when it loads the library (declare), the test-hook headers included."""
    root = os.path.dirname(os.path.dirname(native.CSRC))
    pat = re.compile(r"qa_\w+\.(restype|argtypes)\s*=[^=]")
    files = [os.path.join(root, "__graft_entry__.py")]
    for top in ("quilt_amd", "tests", "scripts"):
        for dirpath, _, names in os.walk(os.path.join(root, top)):
            files += [os.path.join(dirpath, f) for f in names if f.endswith((".py", ".sh", ".R"))]
    assert len(files) > 50
    for f in files:
        if os.path.realpath(f) == os.path.realpath(native.__file__):
            continue
        assert not pat.search(open(f).read()), f"{os.path.relpath(f, root)} declares a prototype of its own"


def test_product_path_never_imports_the_oracle():
    """Nothing under quilt_amd/ may import, link or call the CPU oracle."""
    root = os.path.dirname(native.CSRC)
    pat = re.compile(r"(^\s*(import|from)\s+oracle\b|liboracle|\bqo_[a-z]|#include\s+\".*oracle)", re.M)
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h", "Makefile")):
                src = open(os.path.join(dirpath, f)).read()
                assert not pat.search(src), f"{f} references the oracle"


def test_nipt_block_table_host_logic_matches_oracle():
    """The library's host-side block definition (gibbs_blocks.hpp: smoothing, quantile, peak picking,
    make_gibbs_considers) against the oracle's restatement of gibbs-nipt-block.cpp:366-523 / :1307-1553 on random inputs
    -- no device needed."""
    import ctypes as C
    import numpy as np
    from oracle import oracle as O
    from quilt_amd import native
    lib = native.lib()
    rng = np.random.default_rng(11)
    for trial in range(40):
        G = int(rng.integers(12, 300))
        L_grid = np.cumsum(rng.integers(200, 3000, size=G)).astype(np.int32)
        rate2 = rng.random(G - 1) * rng.choice([0.005, 0.05, 0.5])
        for _ in range(int(rng.integers(0, 6))):
            at = int(rng.integers(0, G - 1))
            rate2[max(at - 2, 0):at + 3] = rng.random() * 1.5
        rate2[-1] = 0
        R = int(rng.integers(5, 400))
        wif = np.sort(rng.integers(0, G, size=R)).astype(np.int32)
        radius = int(rng.choice([500, 5000, 50000]))
        q = float(rng.choice([0.9, 0.95]))
        blocked_ref = O.define_blocked_grids(rate2, L_grid, radius, q)
        ref = O.make_gibbs_considers(blocked_ref, wif)
        arrs = [np.zeros(G, dtype=np.int32) for _ in range(6)]
        n = C.c_int32()
        native.check(lib.qa_nipt_block_table(native.ptr(rate2), native.ptr(L_grid), C.c_int32(G), C.c_int32(radius),
                                             C.c_double(q), native.ptr(wif), C.c_int32(R), *[native.ptr(a) for a in arrs],
                                             C.byref(n)))
        assert np.array_equal(arrs[0], blocked_ref)
        assert n.value == ref["n_blocks"]
        for a, name in zip(arrs[1:5], ("consider_grid_start_0_based", "consider_grid_end_0_based",
                                       "consider_reads_start_0_based", "consider_reads_end_0_based")):
            assert np.array_equal(a[:n.value], ref[name]), name
        assert np.array_equal(arrs[5], ref["consider_grid_where_0_based"])
