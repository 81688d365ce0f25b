"""tools/policy_loop_audit.py's parser on a short synthetic listing (no compiler, no GPU): descriptor fields, loop membership from the compiler's
block comments (a cold block of the function placed between a loop's blocks is not counted), v_mfma and vmcnt(0) counts, one row per body of a
kernel with two tile loops, and the side-by-side table."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import policy_loop_audit as A      # noqa: E402

SYM1 = '_Z13k_policy_mfmaILi10ELi2ELi32ELi0EEv4PolKPKfS2_Pf'
SYM2 = '_Z13k_policy_mfmaILi10ELi2ELi32ELi2EEv4PolKPKfS2_Pf'
LISTING = """
\t.text
%(s1)s: ; @%(s1)s
; %%bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt vmcnt(0)
\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]
\ts_branch .LBB0_3
.LBB0_1:                                ;   in Loop: Header=BB0_3 Depth=1
\tv_mov_b32_e32 v1, 0
.LBB0_2:
\ts_waitcnt vmcnt(0)
\tv_mov_b32_e32 v9, 0
.LBB0_3:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_4 Depth 2
\ts_waitcnt vmcnt(0)
\tglobal_load_dword v7, v[8:9], off
\ts_waitcnt vmcnt(0)
\ts_waitcnt vmcnt(3) lgkmcnt(0)
.LBB0_4:                                ;   Parent Loop BB0_3 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\ts_waitcnt vmcnt(0) lgkmcnt(1)
\ts_cbranch_scc1 .LBB0_4
; %%bb.5:                                ;   in Loop: Header=BB0_3 Depth=1
\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]
\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]
\ts_waitcnt vmcnt(0)
\ts_cbranch_vccnz .LBB0_1
; %%bb.6:
\ts_waitcnt vmcnt(0)
.LBB0_7:                                ; =>This Inner Loop Header: Depth=1
\tv_add_f32_e32 v1, v1, v1
\ts_cbranch_scc1 .LBB0_7
.LBB0_8:                                ; =>This Inner Loop Header: Depth=1
\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]
\ts_cbranch_scc1 .LBB0_8
; %%bb.9:
\ts_endpgm
.Lfunc_end0:
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel %(s1)s
\t\t.amdhsa_private_segment_fixed_size 12
\t\t.amdhsa_next_free_vgpr 212
\t\t.amdhsa_next_free_sgpr 96
\t.end_amdhsa_kernel
\t.text
%(s2)s: ; @%(s2)s
\tv_mov_b32_e32 v0, 0
\ts_endpgm
.Lfunc_end1:
\t.amdhsa_kernel %(s2)s
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr 110
\t.end_amdhsa_kernel
""" % dict(s1=SYM1, s2=SYM2)


def test_parse_counts():
    k1, k2 = A.parse(LISTING)
    assert (k1['kernel'], k1['vgpr'], k1['priv']) == ('k_policy_mfma<10,2,32,0>', 212, 12)
    assert (k2['kernel'], k2['vgpr'], k2['priv'], k2['loops']) == ('k_policy_mfma<10,2,32,2>', 110, 0, [])
    # loop BB0_3: its header block, the nested loop, %bb.5 and the block .LBB0_1 placed above the header; .LBB0_2 (no loop comment) and %bb.6 are outside.
    # The wait at the top of the header block, ahead of the loop's first load, counts in vm0_loop but not in vm0_head.  The loop without a v_mfma (BB0_7) has
    # no row; BB0_8 is the second body.
    assert k1['loops'] == [dict(mfma=2, vm0_head=2, vm0_loop=4, lines=11), dict(mfma=1, vm0_head=0, vm0_loop=0, lines=2)]


def test_tables():
    new = A.parse(LISTING)
    lines = A.table(new).splitlines()
    assert lines[0].split() == ['kernel', 'loop'] + list(A.COLS)
    assert lines[1].split() == ['k_policy_mfma<10,2,32,0>', '0', '212', '12', '2', '2', '4', '11']
    assert lines[2].split()[:4] == ['k_policy_mfma<10,2,32,0>', '1', '212', '12']
    assert lines[3].split() == ['k_policy_mfma<10,2,32,2>', '0', '110', '0', '-', '-', '-', '-']
    old = A.parse(LISTING.replace('fixed_size 12', 'fixed_size 0'))
    side = A.table(new, old).splitlines()
    assert '0 | 12' in side[1] and '212 | 212' in side[1] and len(side) == 4


def test_flags_are_the_makefiles():
    mk = open(os.path.join(A.CSRC, 'Makefile')).read()
    cxx = next(l for l in mk.splitlines() if l.startswith('CXXFLAGS'))
    for f in A.FLAGS:
        assert f.replace('gfx950', '$(ARCH)') in cxx, f
