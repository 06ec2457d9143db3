"""CPU: the parser and the rule of scripts/check_ring_waits.py on three hand-written ISA texts -- a ring loop with one wait per
group, a ring loop that drains its gathers (vmcnt(0) in front of all 24 MFMAs of the iteration, what the F-solve kernels compiled
to before the prologue's load order was pinned) and a kernel without a ring.  No compiler runs here."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    'check_ring_waits', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'scripts', 'check_ring_waits.py'))
crw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(crw)

MFMA = '\tv_mfma_f32_16x16x4_f32 v[110:113], v114, v114, v[110:113]\n'


def group(wait, n=6):
    return '\ts_waitcnt vmcnt(%d)\n' % wait + MFMA * n + '\tbuffer_load_dwordx3 v[114:116], v114, s[44:47], 0 offen\n'


# compiler output (-S): a prologue, the loop (header .LBB0_2, row end in a block of its own), the factorisation behind it
EXACT = ('_ZN4trmf18fsolve_quad_kernelILi3ELi40EEEvPKjS2_PKfS4_Pfjjifjj: ; @_ZN4trmf18fsolve_quad_kernelILi3ELi40EEEvPKjS2_PKfS4_Pfjjifjj\n'
         '; %bb.0:\n'
         '\ts_load_dwordx8 s[4:11], s[0:1], 0x0\n'
         '\ts_waitcnt lgkmcnt(0)\n'
         '\ts_cbranch_scc1 .LBB0_5\n'
         '.LBB0_2:                                ; =>This Loop Header: Depth=1\n'
         + group(3) + group(5) + group(5) + group(5) +
         '\ts_cbranch_scc1 .LBB0_4\n'
         '; %bb.3:                                ;   in Loop: Header=BB0_2 Depth=1\n'
         '\tds_write_b128 v1, v[110:113]\n'
         '\ts_waitcnt lgkmcnt(0)\n'
         '.LBB0_4:                                ;   in Loop: Header=BB0_2 Depth=1\n'
         '\ts_cmp_lt_i32 s17, 0\n'
         '\ts_cbranch_scc0 .LBB0_2\n'
         '.LBB0_5:\n'
         '\ts_waitcnt vmcnt(0)\n'
         '\tv_mfma_f32_4x4x1_16b_f32 v[0:3], v4, v5, v[0:3] cbsz:2 abid:1\n'
         '\ts_endpgm\n'
         '.Lfunc_end0:\n')

# disassembler output (llvm-objdump -d --symbolize-operands): the same loop with one merged wait
DRAIN = ('000000000000e200 <_ZN4trmf18fsolve_quad_kernelILi3ELi40EEEvPKjS2_PKfS4_Pfjjifjj>:\n'
         '\ts_load_dwordx8 s[4:11], s[0:1], 0x0                      // 00000000E200: C00E0100 00000000\n'
         '\ts_cbranch_scc1 L1                                        // 00000000E208: BF850040\n'
         '000000000000e20c <L0>:\n'
         '\ts_waitcnt vmcnt(0)                                       // 00000000E20C: BF8C0F70\n'
         + MFMA * 24 +
         '\tbuffer_load_dwordx3 v[114:116], v114, s[44:47], 0 offen  // 00000000E300: E0581000 800B7272\n'
         '\ts_cmp_lt_i32 s17, 0                                      // 00000000E308: BF048011\n'
         '\ts_cbranch_scc0 L0                                        // 00000000E30C: BF84FFBF\n'
         '000000000000e310 <L1>:\n'
         '\ts_endpgm                                                 // 00000000E310: BF810000\n')

# a loop with loads and waits but no 16x16x4 MFMA, and 16x16x4 MFMAs outside any loop
NO_RING = ('_ZN4trmf11loss_kernelILi3EEEvPKjS2_PKfS4_S4_Pdjj:\n'
           '.LBB3_1:\n'
           '\tbuffer_load_dwordx3 v[4:6], v7, s[8:11], 0 offen\n'
           '\ts_waitcnt vmcnt(0)\n'
           '\tv_fma_f32 v1, v4, v5, v1\n'
           '\ts_cbranch_scc1 .LBB3_1\n'
           '; %bb.2:\n'
           '\ts_waitcnt vmcnt(0)\n'
           + MFMA * 24 +
           '\ts_endpgm\n')


def test_exact_loop_passes():
    res = crw.check_text(EXACT)
    assert [(name, summary, bad) for name, summary, bad, _ in res] == [('fsolve_quad_kernel<3,40>', '[3] M6 [5] M6 [5] M6 [5] M6', [])]


def test_draining_loop_fails():
    (name, summary, bad, allowed), = crw.check_text(DRAIN)
    assert name == 'fsolve_quad_kernel<3,40>' and summary == '[0] M24' and allowed is None
    assert any('more than 6 MFMAs' in b for b in bad) and any('vmcnt(0)' in b for b in bad)


def test_each_rule_on_its_own():
    # one wait per group, but the first one drains: only the vmcnt(0) rule fires
    text = EXACT.replace('s_waitcnt vmcnt(3)', 's_waitcnt vmcnt(0)')
    (_, summary, bad, _), = crw.check_text(text)
    assert summary == '[0] M6 [5] M6 [5] M6 [5] M6' and len(bad) == 1 and 'vmcnt(0)' in bad[0]
    # groups 1-3 behind one wait that is not a drain: only the group rule fires
    text = EXACT.replace(group(5) * 3, '\ts_waitcnt vmcnt(4)\n' + MFMA * 18)
    (_, summary, bad, _), = crw.check_text(text)
    assert summary == '[3] M6 [4] M18' and len(bad) == 1 and 'more than 6 MFMAs' in bad[0]
    # a wait of the scalar / LDS counters only is not a wait for loads
    text = EXACT.replace(group(5), '\ts_waitcnt lgkmcnt(0)\n' + MFMA * 6, 1)
    (_, summary, bad, _), = crw.check_text(text)
    assert summary == '[3] M12 [5] M6 [5] M6' and bad


def test_groups_in_blocks_of_their_own():
    # row ends at group granularity: groups 1..3 behind a scalar branch each, the blocks are shown apart and judged as one sequence
    text = EXACT
    for i, lab in enumerate(('.LBB0_10', '.LBB0_11', '.LBB0_12')):
        text = text.replace(group(5), '\ts_cbranch_scc1 %s\n; %%bb.%d:\n\ts_waitcnt vmcnt(6)\n' % (lab, 20 + i) + MFMA * 6 + lab + ':\n'
                            '\tbuffer_load_dwordx3 v[114:116], v114, s[44:47], 0 offen\n', 1)
    (_, summary, bad, _), = crw.check_text(text)
    assert summary == '[3] M6 || [6] M6 || [6] M6 || [6] M6' and bad == []
    (_, summary, bad, _), = crw.check_text(text.replace('s_waitcnt vmcnt(6)', 's_waitcnt vmcnt(0)', 1))
    assert summary == '[3] M6 || [0] M6 || [6] M6 || [6] M6' and len(bad) == 1 and 'vmcnt(0)' in bad[0]


def test_waits_in_blocks_without_mfmas_count():
    # the join block behind a skipped group holds the group's reload and, possibly, a wait: it stands in front of the next group
    join = '.LBB0_10:\n\tbuffer_load_dwordx3 v[118:120], v118, s[44:47], 0 offen\n\ts_waitcnt vmcnt(%d)\n\ts_cbranch_scc1 .LBB0_11\n; %%bb.21:\n'
    def loop(join_wait):
        return EXACT.replace(group(5) * 3, '\ts_cbranch_scc1 .LBB0_10\n; %bb.20:\n\ts_waitcnt vmcnt(5)\n' + MFMA * 6 + join % join_wait
                             + '\ts_waitcnt vmcnt(5)\n' + MFMA * 6 + '.LBB0_11:\n\tbuffer_load_dwordx3 v[122:124], v122, s[44:47], 0 offen\n')
    (_, summary, bad, _), = crw.check_text(loop(5))
    assert summary == '[3] M6 || [5] M6 || [5] || [5] M6' and bad == []
    (_, summary, bad, _), = crw.check_text(loop(0))
    assert summary == '[3] M6 || [5] M6 || [0] || [5] M6' and len(bad) == 1 and 'vmcnt(0)' in bad[0]
    # MFMAs of two blocks with no wait between them are one run
    text = loop(5).replace('; %bb.21:\n\ts_waitcnt vmcnt(5)\n', '; %bb.21:\n').replace('\ts_waitcnt vmcnt(5)\n\ts_cbranch_scc1 .LBB0_11', '\ts_cbranch_scc1 .LBB0_11')
    (_, summary, bad, _), = crw.check_text(text)
    assert summary == '[3] M6 || [5] M6 || M6' and len(bad) == 1 and 'more than 6 MFMAs' in bad[0]


def test_a_drain_with_a_second_wait_behind_it_still_fails():
    text = EXACT.replace('\ts_waitcnt vmcnt(3)\n', '\ts_waitcnt vmcnt(0)\n\ts_waitcnt vmcnt(5)\n')
    (_, summary, bad, _), = crw.check_text(text)
    assert summary == '[0] [5] M6 [5] M6 [5] M6 [5] M6' and len(bad) == 1 and 'vmcnt(0)' in bad[0]
    # behind the loop's last MFMAs a vmcnt(0) delays nothing of this iteration
    text = EXACT.replace('\ts_cbranch_scc1 .LBB0_4\n', '\ts_waitcnt vmcnt(0)\n\ts_cbranch_scc1 .LBB0_4\n')
    (_, summary, bad, _), = crw.check_text(text)
    assert summary == '[3] M6 [5] M6 [5] M6 [5] M6 [0]' and bad == []


def test_kernel_without_ring_is_ignored():
    assert crw.check_text(NO_RING) == []
    assert [r[0] for r in crw.check_text(NO_RING + EXACT)] == ['fsolve_quad_kernel<3,40>']


def test_allow_list_and_exit_codes(tmp_path, monkeypatch, capsys):
    files = {}
    for name, text in (('exact', EXACT), ('drain', DRAIN), ('none', NO_RING)):
        files[name] = str(tmp_path / (name + '.s'))
        open(files[name], 'w').write(text)
    assert crw.main([files['exact']]) == 0
    assert crw.main([files['exact'], files['drain']]) == 1
    assert crw.main([files['none']]) == 2                        # nothing to look at: the build's inputs are wrong
    monkeypatch.setitem(crw.ALLOW, 'fsolve_quad_kernel<3,40>', 'test')
    assert crw.main([files['drain']]) == 0
    assert '(allowed: test)' in capsys.readouterr().out


def test_pretty_names():
    assert crw.pretty('_ZN4trmf13gram_x_kernelILi3ELb1ELb0EEEvPKjS2_PKfS4_PfS5_jjijmj') == 'gram_x_kernel<3,true,false>'
    assert crw.pretty('_ZN4trmf18fsolve_mfma_kernelILi4ELi64EEEvPKjS2_PKdS4_Pdjjidjj') == 'fsolve_mfma_kernel<4,64>'
    assert crw.pretty('main') == 'main'
