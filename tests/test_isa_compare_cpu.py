"""tools/isa_compare.py on hand-written assembly: the tool that shows a source move left the
device code alone must call a move a move and a change a change."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_compare  # noqa: E402


def _func(sym, ordinal, operand="v1", tmp=7):
    """A kernel as the compiler prints it: label to .Lfunc_end, the descriptor inside."""
    return f"""	.globl	{sym}
	.type	{sym},@function
{sym}:
.Lfunc_begin{ordinal}:
	s_cbranch_scc1 .LBB{ordinal}_2
.Ltmp{tmp}:
	v_add_f64 v[2:3], v[2:3], {operand}
.LBB{ordinal}_2:                              ;   in Loop: Header=BB{ordinal}_2 Depth=1
	s_endpgm
	.amdhsa_kernel {sym}
		.amdhsa_next_free_vgpr 4
	.end_amdhsa_kernel
.Lfunc_end{ordinal}:
	.size	{sym}, .Lfunc_end{ordinal}-{sym}
"""


TAIL = """	.ident	"clang version {v}"
__hip_cuid_{v}:
	.globl	__hip_cuid_{v}
"""


def _run(tmp_path, a, b, ordered=False):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a)
    pb.write_text(b)
    out = io.StringIO()
    rc = isa_compare.compare(str(pa), str(pb), ordered, out)
    return rc, out.getvalue()


def test_swapped_functions_are_equal_unless_ordered(tmp_path):
    a = _func("k_one", 0, tmp=3) + _func("k_two", 1, "v5", tmp=4) + TAIL.format(v="aa")
    b = _func("k_two", 0, "v5", tmp=11) + _func("k_one", 1, tmp=12) + TAIL.format(v="bb")
    rc, text = _run(tmp_path, a, b)
    assert rc == 0 and "identical: 2 functions, 2 kernel descriptors" in text
    rc, text = _run(tmp_path, a, b, ordered=True)
    assert rc == 1 and "order differs" in text and "k_one" in text
    rc, _ = _run(tmp_path, a, a, ordered=True)
    assert rc == 0


def test_changed_operand_is_reported_under_its_symbol(tmp_path):
    a = _func("k_one", 0) + _func("k_two", 1)
    b = _func("k_one", 0) + _func("k_two", 1, "v9")
    rc, text = _run(tmp_path, a, b)
    assert rc == 1
    assert "differs: k_two" in text and "v9" in text
    assert "k_one" not in text and "only in" not in text


def test_missing_kernel_is_reported(tmp_path):
    a = _func("k_one", 0) + _func("k_two", 1)
    rc, text = _run(tmp_path, a, _func("k_one", 0))
    assert rc == 1
    assert "only in A: k_two" in text and "only in A: kernel descriptor k_two" in text
    rc, text = _run(tmp_path, _func("k_two", 0), a)
    assert rc == 1 and "only in B: k_one" in text and "differs" not in text
