"""tools/listing_diff.py on two tiny made-up listings (text only; no compiler, no GPU)."""
import importlib.util
import io
import os

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "listing_diff.py")
_SPEC = importlib.util.spec_from_file_location("listing_diff", _PATH)
listing_diff = importlib.util.module_from_spec(_SPEC)
_SPEC.loader.exec_module(listing_diff)

# one kernel as `hipcc -S` lays it out: label, instructions, resource block, end label
LISTING = """\
\t.globl\t{sym} ; -- Begin function {sym}
{sym}: ; @{sym}
; %bb.0:
\ts_load_dword s0, s[4:5], 0x0
\ts_cbranch_scc1 .LBB{n}_2
\ts_getpc_b64 s[2:3]
.Lpost_getpc{n}:
\ts_add_u32 s2, s2, (.LBB{n}_2-.Lpost_getpc{n})&4294967295
; %bb.1:
\tv_mov_b32_e32 v0, {imm}
.LBB{n}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {sym}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
.Lfunc_end{n}:
\t.size\t{sym}, .Lfunc_end{n}-{sym}
"""
# the same kernel before and after a move: another label number, its argument type in another namespace
OLD_SYM = "_ZN12_GLOBAL__N_16k_copyILi4ELb1EEEvNS_4ArgsE"
NEW_SYM = "_ZN12_GLOBAL__N_16k_copyILi4ELb1EEEvN3rsk4ArgsE"


def write(tmp_path, name, **kw):
    p = tmp_path / name
    p.write_text(LISTING.format(**{"imm": 0, "vgpr": 4, **kw}))
    return [str(p)]


def report(old, new):
    out = io.StringIO()
    bad = listing_diff.compare(listing_diff.kernels(old), listing_diff.kernels(new), out)
    return bad, out.getvalue()


def test_listing_diff(tmp_path):
    assert listing_diff.kernel_key(OLD_SYM) == listing_diff.kernel_key(NEW_SYM) == "k_copy<i4,b1>"
    old = write(tmp_path, "old.s", sym=OLD_SYM, n=7)
    # equal bodies under different label numbers and another mangled argument type: equal
    bad, text = report(old, write(tmp_path, "moved.s", sym=NEW_SYM, n=0))
    assert bad == 0 and "1 kernels equal, 0 different" in text, text
    # one changed operand: different, with the line in the diff
    bad, text = report(old, write(tmp_path, "operand.s", sym=NEW_SYM, n=0, imm=1))
    assert bad == 1 and "DIFFERENT k_copy<i4,b1>: instructions" in text and "+\tv_mov_b32_e32 v0, 1" in text, text
    # one changed resource figure: different
    bad, text = report(old, write(tmp_path, "vgpr.s", sym=NEW_SYM, n=0, vgpr=5))
    assert bad == 1 and "DIFFERENT k_copy<i4,b1>: resources" in text, text
    # another template argument: two unpaired kernels
    bad, text = report(old, write(tmp_path, "other.s", sym=NEW_SYM.replace("Li4E", "Li2E"), n=0))
    assert bad == 2 and text.count("UNPAIRED") == 2, text
