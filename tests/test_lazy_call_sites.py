"""Every call of the G1 law's loads, stores, additions, doublings and conversions in the device units, classified -
under every name the sources give the law: G1L, a template parameter G, msm.hip's G1S = G1LT<0> (the scan resolves
`using X = G1LT<..>` itself, so a new alias cannot slip past), the field load of the quad kernels (G1S::F::load), the
quad-lane form (QD = QuadG1<..>: add, dbl), and C in lagrange_elem29.hpp, where the Lagrange kernels' arithmetic lives
(lagrange.hip itself calls the law only through Lag::; it is scanned so that a direct call would need a row).

tests/test_curve_envelope_host.py proves that the classes of curve29.hpp close under the chains the kernels build; this
table says which class every operand of every call site is in, and who writes the memory a load reads - so that a new
call has to be classified (and its chain shown to close from that class) before it merges.  Classes, as in
tests/cpp/curve_envelope_check.cpp:
    T    table point in memory, canonical (written by store_affine only)
    R    register point of the general law            A    accumulator of the lean forms
    M    bucket memory as store() of this library wrote it (never a caller's words)
    P    register point whose coordinates are products of arbitrary 32-byte images (from_ext of a caller's words)
    inf  the literal point at infinity
No load of the law reads memory that a caller writes: caller words enter through Fq29::from_ext (a product) in
msm_precompute_kernel, msm_var_convert, g1_sum_kernel, g1_sum_ranks_kernel and load_abi.  A load that did would have the
class "any 32-byte image"; the envelope closes from that class too ("M any image" in the golden table).
(`-m "not gpu"`)"""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cap_amd", "csrc")
UNITS = ("msm.hip", "capgpu.hip", "comm.hip", "verify_dev.hip", "lagrange.hip", "lagrange_elem29.hpp")
OPS = r"(load|store_affine|store|add_affine_pair|add_mixed|add_acc|add|madd_acc|dbl_affine|dbl|to_affine|to_jac_ext|to_\w+)"
NOT_A_NAME = ("__launch_bounds__", "__attribute__", "defined")


def call_pattern(text):
    """the calls of the law in a source text, under every name the text gives it: G1L and a template parameter G, any
    `using X = G1LT<..>` / `using X = .. LagCurve<..>::C` (msm.hip: G1S; lagrange_elem29.hpp: C), a literal G1LT<..>::,
    the field's load and pack through such a name (X::F::load, X::F::pack: the quad kernels' bucket loads and stores), and add / dbl of any
    `using Y = QuadG1<..>` (the quad-lane form of the same law)"""
    law = {"G1L", "G"} | set(re.findall(r"using\s+(\w+)\s*=\s*(?:typename\s+)?(?:G1LT|LagCurve)<", text))
    quad = set(re.findall(r"using\s+(\w+)\s*=\s*QuadG1<", text))
    names = "|".join(sorted(law))
    pat = rf"\b(?:{names}|G1LT<[^>]*>)::{OPS}\s*\(|\b(?:{names})::F::(load|pack)\s*\("
    if quad:
        pat += rf"|\b(?:{'|'.join(sorted(quad))})::(add|dbl)\s*\("
    return re.compile(pat)


def scan(path):
    """-> {(function, call, n)}: the calls of the law in one source file, comments left out; calls of the field's load
    and pack are named "F::load" / "F::pack", those of the quad form "quad add" / "quad dbl" """
    found, fn, counts = set(), None, {}
    with open(path) as f:
        text = f.read()
    call = call_pattern(text)
    for line in text.split("\n"):
        code = line.split("//")[0]
        starts = line[:1] not in " \t}#/" and line != ""                # a definition starts in column 0 ...
        member = line.startswith("  static ") and not line.startswith("   ")   # ... or is a static member of a struct
        if (starts or member) and "(" in code:
            names = [n for n in re.findall(r"\b(\w+)\s*\(", code) if n not in NOT_A_NAME]
            if names:
                fn = names[0]
        for m in call.finditer(code):
            what = m.group(1) or ("F::" + m.group(2) if m.group(2) else "quad " + m.group(3))
            counts[(fn, what)] = counts.get((fn, what), 0) + 1
            found.add((fn, what, counts[(fn, what)]))
    return found

WORKSPACE = "this library: store() in msm_accumulate / msm_combine* / msm_reduce_*"
TABLE_MEM = "this library: store_affine() in msm_precompute_kernel / msm_var_convert"
REG = "registers"
LAG_MEM = "this library: store() in lag_load / lag_stage"
SRS_MEM = "this library: store_affine() in msm_precompute_kernel (window 0 of the SRS table)"
# (unit, function, call, n-th such call in the function): (classes of the operands, who writes what it reads)
SITES = {
    ("msm.hip", "msm_precompute_kernel", "store_affine", 1): (("canonical x, y",), REG),
    ("msm.hip", "msm_precompute_kernel", "dbl", 1): (("R",), REG),
    ("msm.hip", "msm_precompute_kernel", "to_affine", 1): (("R",), REG),
    ("msm.hip", "msm_precompute_kernel", "store_affine", 2): (("to_affine's products",), REG),
    ("msm.hip", "add_tree", "add_acc", 1): (("A or M", "A or M"), REG),
    ("msm.hip", "add_tree", "add", 1): (("A or M", "A or M"), REG),
    ("msm.hip", "msm_combine_wave", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_combine_wave", "load", 2): (("M",), WORKSPACE),
    ("msm.hip", "msm_combine_wave", "store", 1): (("A",), REG),
    ("msm.hip", "msm_accumulate", "load", 1): (("T",), TABLE_MEM),
    ("msm.hip", "msm_accumulate", "load", 2): (("T",), TABLE_MEM),
    ("msm.hip", "msm_accumulate", "load", 3): (("T",), TABLE_MEM),
    ("msm.hip", "msm_accumulate", "add_affine_pair", 1): (("T", "T"), REG),
    ("msm.hip", "msm_accumulate", "madd_acc", 1): (("A", "T"), REG),
    ("msm.hip", "msm_accumulate", "add_mixed", 1): (("A or inf", "T or inf"), REG),
    ("msm.hip", "msm_accumulate", "store", 1): (("A",), REG),
    ("msm.hip", "msm_accumulate", "store", 2): (("A",), REG),
    ("msm.hip", "msm_reduce_segments", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_segments", "load", 2): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_segments", "add_acc", 1): (("A", "A"), REG),
    ("msm.hip", "msm_reduce_segments", "add", 1): (("A", "A"), REG),
    ("msm.hip", "msm_reduce_segments", "add_acc", 2): (("A", "A"), REG),
    ("msm.hip", "msm_reduce_segments", "add", 2): (("A", "A"), REG),
    ("msm.hip", "msm_reduce_segments", "store", 1): (("A",), REG),
    ("msm.hip", "msm_reduce_segments", "store", 2): (("A",), REG),
    ("msm.hip", "mul_small", "dbl", 1): (("A",), REG),
    ("msm.hip", "mul_small", "add", 1): (("R or inf", "A"), REG),
    ("msm.hip", "msm_combine", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_combine", "load", 2): (("M",), WORKSPACE),
    ("msm.hip", "msm_combine", "add", 1): (("A", "A"), REG),
    ("msm.hip", "msm_combine", "store", 1): (("A",), REG),
    ("msm.hip", "msm_reduce_bits", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_bits", "load", 2): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_bits", "load", 3): (("M",), "this kernel: store() into LDS two lines above"),
    ("msm.hip", "msm_reduce_bits", "store", 1): (("A",), REG),
    ("msm.hip", "msm_reduce_bits", "store", 2): (("A",), REG),
    ("msm.hip", "msm_reduce_grid", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid", "load", 2): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid", "store", 1): (("A",), REG),
    ("msm.hip", "msm_fill_inf", "to_jac_ext", 1): (("inf",), REG),
    ("msm.hip", "msm_var_convert", "store_affine", 1): (("canonical x, y",), REG),
    ("capgpu.hip", "g1_sum_kernel", "add", 1): (("R or inf", "P or inf"), REG),
    ("capgpu.hip", "g1_sum_kernel", "add", 2): (("R or inf", "R or inf"), REG),
    ("capgpu.hip", "g1_sum_kernel", "to_jac_ext", 1): (("R or inf",), REG),
    ("comm.hip", "g1_sum_ranks_kernel", "add", 1): (("R or inf", "P or inf"), REG),
    ("comm.hip", "g1_sum_ranks_kernel", "add", 2): (("R or inf", "R or inf"), REG),
    ("comm.hip", "g1_sum_ranks_kernel", "to_jac_ext", 1): (("R or inf",), REG),
    ("verify_dev.hip", "k_verify_terms", "add", 1): (("R or inf", "R or inf"), REG),
    ("verify_dev.hip", "k_verify_terms", "add", 2): (("R or inf", "R or inf"), REG),
    ("verify_dev.hip", "k_verify_terms", "add", 3): (("R or inf", "R or inf"), "this kernel: LDS copies of registers"),
    ("verify_dev.hip", "k_verify_terms", "add", 4): (("R or inf", "R or inf"), "this kernel: LDS copies of registers"),
    ("verify_dev.hip", "k_verify_terms", "to_affine", 1): (("R",), REG),
    # the finishing kernels of msm.hip (the law as G1S = G1LT<0>, and its quad-lane form QD): every g1_xyzz they read -
    # buckets, segment and grid sums, partial sums, the LDS and global hand-over slots - was written by store() or the
    # quad kernels' pack of a register point in this library; a quad holds the same point, one coordinate per lane
    # the Lagrange key builder (lagrange_elem29.hpp, the law as C): the transform's array holds what load_point and
    # butterfly stored; the SRS rows are table points
    ("lagrange_elem29.hpp", "butterfly", "add", 1): (("M or R", "R or M"), REG),
    ("lagrange_elem29.hpp", "butterfly", "add", 2): (("M or R", "R or M"), REG),
    ("lagrange_elem29.hpp", "butterfly", "load", 1): (("M",), LAG_MEM),
    ("lagrange_elem29.hpp", "butterfly", "load", 2): (("M",), LAG_MEM),
    ("lagrange_elem29.hpp", "butterfly", "store", 1): (("R or M",), REG),
    ("lagrange_elem29.hpp", "butterfly", "store", 2): (("R or M",), REG),
    ("lagrange_elem29.hpp", "finish", "add_mixed", 1): (("R", "T"), REG),
    ("lagrange_elem29.hpp", "finish", "load", 1): (("M",), LAG_MEM),
    ("lagrange_elem29.hpp", "finish", "load", 2): (("T",), SRS_MEM),
    ("lagrange_elem29.hpp", "finish", "load", 3): (("T",), SRS_MEM),
    ("lagrange_elem29.hpp", "finish", "to_affine", 1): (("R",), REG),
    ("lagrange_elem29.hpp", "load_point", "load", 1): (("T",), SRS_MEM),
    ("lagrange_elem29.hpp", "load_point", "store", 1): (("R",), REG),
    ("lagrange_elem29.hpp", "scalar_mul", "add", 1): (("R or inf", "R or M"), REG),
    ("lagrange_elem29.hpp", "scalar_mul", "add", 2): (("R or inf", "R or M"), REG),
    ("lagrange_elem29.hpp", "scalar_mul", "dbl", 1): (("R or M or inf",), REG),
    ("lagrange_elem29.hpp", "scalar_mul", "dbl", 2): (("R or M or inf",), REG),
    ("lagrange_elem29.hpp", "scalar_mul", "dbl", 3): (("R or M or inf",), REG),
    ("msm.hip", "msm_combine_quad", "quad add", 1): (("A or inf", "A or inf"), REG),
    ("msm.hip", "msm_combine_quad", "quad add", 2): (("A or inf", "A or inf"), REG),
    ("msm.hip", "msm_reduce_bits_final", "dbl", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_bits_final", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_bits_final", "load", 2): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_bits_final", "store", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_bits_final", "store", 2): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_bits_final", "store", 3): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_bits_final", "to_jac_ext", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_final", "add", 1): (("A or inf", "A or inf"), REG),
    ("msm.hip", "msm_reduce_final", "add", 2): (("A or inf", "A or inf"), REG),
    ("msm.hip", "msm_reduce_final", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_final", "load", 2): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_final", "store", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_final", "store", 2): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_final", "store", 3): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_final", "to_jac_ext", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_final_quad", "to_jac_ext", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final", "dbl", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final", "dbl", 2): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final", "load", 2): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final", "load", 3): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final", "load", 4): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final", "load", 5): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final", "load", 6): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final", "load", 7): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final", "load", 8): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final", "store", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final", "store", 2): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final", "store", 3): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final", "store", 4): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final", "to_jac_ext", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final_quad", "F::load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final_quad", "quad add", 1): (("A or inf", "A or inf"), REG),
    ("msm.hip", "msm_reduce_grid_final_quad", "quad add", 2): (("A or inf", "A or inf"), REG),
    ("msm.hip", "msm_reduce_grid_final_quad", "quad dbl", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final_quad", "store", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final_quad", "to_jac_ext", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final_small", "dbl", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final_small", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final_small", "load", 2): (("M",), WORKSPACE),
    ("msm.hip", "msm_reduce_grid_final_small", "store", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final_small", "store", 2): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_final_small", "to_jac_ext", 1): (("A or inf",), REG),
    ("msm.hip", "msm_reduce_grid_quad", "quad add", 1): (("A or inf", "A or inf"), REG),
    ("msm.hip", "msm_reduce_grid_quad", "quad add", 2): (("A or inf", "A or inf"), REG),
    ("msm.hip", "msm_sum_parts", "add", 1): (("A or inf", "A or inf"), REG),
    ("msm.hip", "msm_sum_parts", "load", 1): (("M",), WORKSPACE),
    ("msm.hip", "msm_sum_parts", "to_jac_ext", 1): (("A or inf",), REG),
    ("msm.hip", "msm_var_horner", "store", 1): (("A or inf",), REG),
    ("msm.hip", "msm_var_horner", "to_jac_ext", 1): (("A or inf",), REG),
    ("msm.hip", "quad_add_call", "quad add", 1): (("A or inf", "A or inf"), REG),
    ("msm.hip", "quad_dbl_call", "quad dbl", 1): (("A or inf",), REG),
    ("msm.hip", "quad_store", "F::pack", 1): (("A",), REG),      # one coordinate of a quad's point per lane: store()
    ("msm.hip", "quad_load", "F::load", 1): (("M",), WORKSPACE),
}
CLASSES = {"T", "R", "A", "M", "P", "inf", "canonical x, y", "to_affine's products"}


def compare(csrc, table):
    """-> (call sites the table lacks, table rows the sources no longer have)"""
    found = {(u,) + k for u in UNITS for k in scan(os.path.join(csrc, u))}
    return sorted(found - set(table)), sorted(set(table) - found)


def test_every_call_site_of_the_law_is_classified():
    missing, stale = compare(CSRC, SITES)
    assert not missing, f"classify these calls in tests/test_lazy_call_sites.py (operand classes, who writes the " \
                        f"memory): {missing}"
    assert not stale, f"these rows no longer match a call in the sources: {stale}"
    for key, (operands, writer) in SITES.items():
        assert writer and operands, key
        for o in operands:
            assert all(part in CLASSES for part in o.split(" or ")), (key, o)
        if key[2] == "load":                                            # a load names the writer of its memory
            assert writer.startswith("this "), key


# The finishing kernels are restated in tests/cpp/curve_envelope_check.cpp as ONE closure ("folds", and with the quad
# form "folds with the quad form"): points loaded from bucket memory, summed with add_tree (add_acc, add) and add,
# doubled, stored and loaded again, in any order.  That bounds a kernel only while the kernel uses nothing else.
FOLD_CLOSURE = {"load", "F::load", "store", "F::pack", "add", "add_acc", "dbl", "to_jac_ext", "quad add", "quad dbl"}
FOLD_KERNELS = {"add_tree", "mul_small", "msm_combine_wave", "msm_combine", "msm_combine_quad", "msm_reduce_bits",
                "msm_reduce_bits_final", "msm_reduce_grid", "msm_reduce_grid_final", "msm_reduce_grid_final_small",
                "msm_reduce_grid_quad", "msm_reduce_grid_final_quad", "msm_reduce_final", "msm_reduce_final_quad",
                "msm_sum_parts", "msm_var_horner", "quad_load", "quad_store", "quad_add_call", "quad_dbl_call"}
CHAIN_KERNELS = {"msm_accumulate", "msm_reduce_segments", "msm_precompute_kernel", "msm_fill_inf", "msm_var_convert"}


def test_the_fold_closure_holds_every_operation_its_kernels_use():
    """every function of msm.hip that calls the law is one of the kernels behind the fold closure - and those use no
    operation outside the closure's set: a lean or mixed addition in one of them has to be restated first - or one of
    CHAIN_KERNELS: msm_accumulate, msm_reduce_segments and msm_precompute_kernel have a chain of their own in the
    envelope program; msm_fill_inf (to_jac_ext of infinity) and msm_var_convert (store_affine of canonical values) are
    a single operation each and are covered by that operation's row.  A new function has to be put in one of the sets."""
    used = {}
    for fn, call, _n in scan(os.path.join(CSRC, "msm.hip")):
        used.setdefault(fn, set()).add(call)
    assert set(used) == FOLD_KERNELS | CHAIN_KERNELS, set(used) ^ (FOLD_KERNELS | CHAIN_KERNELS)
    for fn in sorted(FOLD_KERNELS):
        assert used[fn] <= FOLD_CLOSURE, (fn, used[fn] - FOLD_CLOSURE)


def test_the_scan_notices_a_new_call_and_a_missing_row(tmp_path):
    for u in UNITS:
        with open(os.path.join(CSRC, u)) as f:
            text = f.read()
        if u == "msm.hip":
            text = text.replace("  g1x T = S;\n", "  g1x T = S;\n  const g1x extra = G1L::load(bk[0]);\n", 1)
            # the law under its other names: the alias of msm.hip, a literal instantiation, a new alias
            text = text.replace("  g1x suf = S;  // inclusive suffix sum over lanes\n",
                                "  g1x suf = S;\n  const g1x e1 = G1S::load(sp[0]);\n  const g1x e2 = G1LT<1>::dbl(e1);\n", 1)
            text = text.replace("using G1S = G1LT<0>;\n", "using G1S = G1LT<0>;\nusing G1New = G1LT<1>;\n", 1)
            text = text.replace("  r = wave_sum<G1S>(r);\n", "  r = wave_sum<G1S>(G1New::add(r, e2));\n", 1)
            assert all(x in text for x in ("extra = G1L::load", "e1 = G1S::load", "G1LT<1>::dbl(e1)", "G1New::add(r, e2)"))
        (tmp_path / u).write_text(text)
    missing, stale = compare(str(tmp_path), SITES)
    assert missing == [("msm.hip", "msm_reduce_final", "add", 3), ("msm.hip", "msm_reduce_final", "dbl", 1),
                       ("msm.hip", "msm_reduce_final", "load", 3), ("msm.hip", "msm_reduce_segments", "load", 3)]
    assert not stale
    fewer = dict(SITES)
    del fewer[("capgpu.hip", "g1_sum_kernel", "add", 2)]
    del fewer[("msm.hip", "msm_sum_parts", "load", 1)]
    missing, stale = compare(CSRC, fewer)
    assert missing == [("capgpu.hip", "g1_sum_kernel", "add", 2), ("msm.hip", "msm_sum_parts", "load", 1)] and not stale
    # a comment that mentions a call is no call
    (tmp_path / "msm.hip").write_text("// G1L::load(x)\nvoid f() {\n  // G1L::add(a, b)\n}\n")
    assert scan(str(tmp_path / "msm.hip")) == set()
