"""The route plan of the Huffman and canonical paths (gf_internal_route_plan, gvrs_api_route.hip), on the CPU: which k_huffman_decode
build, fast-run form, k_canon_decode build, pre-pass form, roomy-run form and encoder form every tile shape of the sweep selects.
The plan is what encodeBatchDev and decodeBatchDev launch (they check their launchers' report against it), so this pins the
dispatch: the inline decisions it replaced, restated below, must agree with it on the whole sweep; the anchors the code
comments give must hold; every instantiation must be reachable; and the edges must sit where the constants say."""
import pytest

import route_plan as rp
from route_plan import KIND_CANON, KIND_HUFFMAN, KIND_RAW_M32

STEP, LDS_PER_CU = 1280, 160 * 1024


def _wgs_per_cu(lds, cap):
    n = LDS_PER_CU // ((lds + STEP - 1) // STEP * STEP)
    return min(n, cap)


def _lds_m32(r, c):
    """gf_huffman_decode_lds_m32 (gvrs_decode.hip)"""
    cells = r * c
    return (min(max(cells + cells // 8 + 512, 8192), 98304) + 31) // 32 * 32


def _old_huffman_threads(r, c, m32, lean):
    """decodeBatchDev before the plan: the k_huffman_decode build from the LDS of one workgroup of each build"""
    L = rp.lib()
    w256 = 4 * _wgs_per_cu(L.gf_internal_decode_lds_per_wg(0, r, c, m32, 0), 8)
    w512 = 8 * _wgs_per_cu(L.gf_internal_decode_lds_per_wg(1, r, c, m32, 0), 4)
    w1024 = 16 * _wgs_per_cu(L.gf_internal_decode_lds_per_wg(2, r, c, m32, 0), 2)
    threads = 512 if 2 * w512 >= 3 * w256 else 256
    if threads == 512 and w1024 >= 2 * w512:
        threads = 1024
    return 1024 if lean else threads


def _old_canon_threads(r, c):
    L = rp.lib()
    w256 = 4 * _wgs_per_cu(L.gf_internal_decode_lds_per_wg(3, r, c, 0, 0), 8)
    w512 = 8 * _wgs_per_cu(L.gf_internal_decode_lds_per_wg(4, r, c, 0, 0), 4)
    return 512 if 2 * w512 >= 3 * w256 and r * c >= 7000 else 256


def _old_decisions(kind, r, c, n_tiles, lean, analysis, roomy_seen):
    """the inline expressions of decodeBatchDev, gf_launch_huffman_decode and encodeBatchDev before the plan, copied"""
    cells = r * c
    m32 = _lds_m32(r, c)
    out = {"fastM32": m32, "prepass": 0, "viaFast": 0, "decThreads": 0, "canonThreads": 0, "ldsM32Roomy": 0,
           "roomyForm": rp.ROOMY_NONE, "leanEncode": int(bool(kind == KIND_HUFFMAN and lean and 6 * cells < (1 << 23)))}
    if kind == KIND_CANON:
        out["prepass"] = 1 if n_tiles <= 4096 else 64
        out["viaFast"] = int(not analysis and r >= 2 and 4 <= c <= 256 and cells + 8 <= m32)
        if out["viaFast"]:
            out["decThreads"] = _old_huffman_threads(r, c, m32, lean)
        if not analysis:
            out["canonThreads"] = _old_canon_threads(r, c)
        return out
    out["decThreads"] = _old_huffman_threads(r, c, m32, lean)
    if kind == KIND_RAW_M32:
        return out
    out["prepass"] = 1 if n_tiles <= 4096 else 64
    if not analysis and not lean:
        roomy = min(98304, (2 * cells + 1024 + 31) & ~31)
        out["ldsM32Roomy"] = roomy if roomy > m32 else 0
    if out["ldsM32Roomy"]:
        likely = roomy_seen != 1
        beside = n_tiles >= 4096 and likely                      # (a context with its side stream)
        no_roomy = not likely and n_tiles < 2048
        out["roomyForm"] = rp.ROOMY_BESIDE if beside else rp.ROOMY_SKIPPED if no_roomy else rp.ROOMY_BEHIND
    return out


def _variants():
    for kind, lean, analysis in ((KIND_HUFFMAN, 0, 0), (KIND_HUFFMAN, 1, 0), (KIND_HUFFMAN, 0, 1), (KIND_RAW_M32, 0, 0),
                                 (KIND_CANON, 0, 0), (KIND_CANON, 1, 0), (KIND_CANON, 0, 1)):
        yield kind, lean, analysis


def test_plan_reproduces_the_inline_decisions_on_the_sweep():
    shapes = rp.sweep()
    assert len(shapes) > 1000
    batches = ((1, 0), (2047, 1), (2048, 1), (4096, 0), (4096, 1), (4096, 5), (4097, 0), (13000, 1))
    n = 0
    for r, c in shapes:
        for kind, lean, analysis in _variants():
            for n_tiles, seen in (batches if kind == KIND_HUFFMAN and not lean and not analysis else batches[:1] + batches[-1:]):
                p = rp.plan(kind, r, c, n_tiles, lean, analysis, seen)
                want = _old_decisions(kind, r, c, n_tiles, lean, analysis, seen)
                got = {k: getattr(p, k) for k in want}
                assert got == want, (kind, r, c, n_tiles, lean, analysis, seen)
                n += 1
    assert n > 20000


def test_plan_bits_name_what_each_form_launches():
    """decBits / encBits against the forms: what decodeBatchDev compares its launchers' report with"""
    for r, c in rp.sweep()[::7]:
        for kind, lean, analysis in _variants():
            p = rp.plan(kind, r, c, 5000, lean, analysis, 0)
            cells = r * c
            if kind == KIND_RAW_M32:
                assert p.decBits == rp.dec_bit(rp.DEC_GENERAL, p.decThreads)
                continue
            if kind == KIND_HUFFMAN:
                want = rp.TREES_64
                if analysis:
                    want |= rp.dec_bit(rp.DEC_ANALYZE, p.decThreads)
                elif lean:
                    want |= rp.dec_bit(rp.DEC_FAST, p.decThreads)
                else:
                    want |= rp.dec_bit(rp.DEC_FAST, p.decThreads) | rp.dec_bit(rp.DEC_GENERAL, p.decThreads)
                    if p.roomyForm in (rp.ROOMY_BESIDE, rp.ROOMY_BEHIND):
                        want |= rp.dec_bit(rp.DEC_FAST_ROOMY, p.decThreads)
                assert p.decBits == want, (r, c, lean, analysis)
                if lean and 6 * cells < (1 << 23):
                    assert p.encBits == rp.ENC_LEAN_T1024 | rp.ENC_FAST | rp.ENC_PACK
                elif 6 * cells < (1 << 23):
                    assert p.encBits == rp.ENC_SPLIT | rp.ENC_PLANE | rp.ENC_PACK | rp.ENC_PACK_RARE
                else:
                    assert p.encBits == rp.ENC_GENERAL | rp.ENC_PACK | (0 if lean else rp.ENC_PACK_RARE)
            else:
                want = rp.LENGTHS_64
                if p.viaFast:
                    want |= rp.dec_bit(rp.DEC_FAST_CANON, p.decThreads)
                want |= rp.CANON_ANALYZE if analysis else rp.CANON_DEC_T512 if p.canonThreads == 512 else rp.CANON_DEC_T256
                assert p.decBits == want, (r, c, lean, analysis)
                assert p.encBits == rp.CANON_ENC_1 | rp.CANON_PACK | (0 if lean else rp.ENC_PLANE)


def test_every_instantiation_is_reachable():
    dom = rp.domains()
    for mode, name in rp.MODES.items():
        for b in rp.BUILDS:
            assert rp.reached(dom, "%s/%d" % (name, b)), "no shape of the sweep launches k_huffman_decode<%s> of the %d-thread build" % (name, b)
    # ... and by a batch, not only by the one-tile path
    for name in ("huffman:DEC_FAST", "huffman:DEC_GENERAL", "huffman:DEC_FAST_ROOMY", "analyze:DEC_ANALYZE", "deflate:DEC_GENERAL",
                 "canon:DEC_FAST_CANON"):
        for b in rp.BUILDS:
            assert dom.get("%s/%d" % (name, b)), (name, b)
    for name in ("k_canon_decode/256", "k_canon_decode/512", "k_canon_decode<true>", "k_huffman_parse_trees<1>",
                 "k_canon_parse_lengths<1>", "k_huffman_encode<true,1>", "k_huffman_encode<true>", "k_huffman_encode<false>",
                 "k_huffman_pack_rare", "encode_t1024", "k_canon_encode<1>"):
        assert rp.reached(dom, name), name
    # k_canon_encode<0> (the one-kernel canonical encoder) is compiled but not on any route: encodeBatchDev always hands the
    # canonical encoder its statistics records.  Should that change, this test and the GPU route tests must cover it.
    assert not rp.reached(dom, "k_canon_encode<0>")
    # the pre-pass's wave-per-64-tiles form by batch size
    assert rp.plan(KIND_HUFFMAN, 120, 150, 4097).decBits & rp.TREES_64
    assert rp.plan(KIND_CANON, 120, 150, 4097).decBits & rp.LENGTHS_64


def test_anchors_of_the_code_comments():
    # CodecHuffman: 120x150 (bench shape) the 512-thread build; 160x160 and more the 1024-thread build; 32x32 and 70x100 256
    assert rp.plan(KIND_HUFFMAN, 120, 150).decThreads == 512
    assert rp.plan(KIND_HUFFMAN, 100, 120).decThreads == 512
    assert rp.plan(KIND_HUFFMAN, 200, 200).decThreads == 1024
    assert rp.plan(KIND_HUFFMAN, 70, 100).decThreads == 256
    assert rp.plan(KIND_HUFFMAN, 32, 32).decThreads == 256
    # squares: the 256-thread build up to 86x86, 512 from 87x87, 1024 from 167x167 -- except 208x208..218x218, where the
    # 1024-thread build's workgroup no longer leaves room for a second one on a CU while the 512-thread build still fits two
    want = {n: 256 if n < 87 else 512 if n < 167 or 208 <= n <= 218 else 1024 for n in range(1, 321)}
    assert {n: rp.plan(KIND_HUFFMAN, n, n).decThreads for n in range(1, 321)} == want
    # the canonical decoder: 90x120 and 100x110 the 512-thread build, 64x64 the 256
    assert rp.plan(KIND_CANON, 90, 120).canonThreads == 512
    assert rp.plan(KIND_CANON, 100, 110).canonThreads == 512
    assert rp.plan(KIND_CANON, 64, 64).canonThreads == 256
    # one tile per call: the widest build
    assert rp.plan(KIND_HUFFMAN, 120, 150, 1, lean=1).decThreads == 1024
    assert rp.plan(KIND_HUFFMAN, 120, 150, 1, lean=1).leanEncode == 1


def test_edges_are_exact():
    # k_canon_decode: 512 threads from 7,000 cells on (where the LDS lets the 512-thread build hold 1.5 times the waves)
    pairs = [((1, 6999), (1, 7000)), ((6999, 1), (7000, 1)), ((3, 2333), (70, 100))]
    assert any(rp.plan(KIND_CANON, *b).canonThreads == 512 for _, b in pairs)
    for a, b in pairs:
        assert rp.plan(KIND_CANON, *a).canonThreads == 256, a
        assert rp.plan(KIND_CANON, *b).canonThreads == _old_canon_threads(*b), b
    assert rp.plan(KIND_CANON, 70, 100).canonThreads == 512
    # the canonical fast run: 2 <= nRows, 4 <= nCols <= 256, cells + 8 within the fast run's M32 buffer
    assert rp.plan(KIND_CANON, 64, 256).viaFast and not rp.plan(KIND_CANON, 64, 257).viaFast
    assert rp.plan(KIND_CANON, 64, 4).viaFast and not rp.plan(KIND_CANON, 64, 3).viaFast
    assert rp.plan(KIND_CANON, 2, 100).viaFast and not rp.plan(KIND_CANON, 1, 100).viaFast
    assert rp.plan(KIND_CANON, 383, 256).viaFast and not rp.plan(KIND_CANON, 384, 256).viaFast
    assert not rp.plan(KIND_CANON, 64, 64, analysis=1).viaFast
    # the one-tile encoder's 1024-thread build: 6 * cells < 2^23
    for r in (1, 2):
        c = rp.LEAN_MAX_CELLS // r
        assert rp.plan(KIND_HUFFMAN, r, c, 1, lean=1).leanEncode == 1
        c2 = -(-(rp.LEAN_MAX_CELLS + 1) // r)
        assert rp.plan(KIND_HUFFMAN, r, c2, 1, lean=1).leanEncode == 0
        assert rp.plan(KIND_HUFFMAN, r, c2, 1, lean=1).encBits & rp.ENC_GENERAL
    assert not rp.plan(KIND_HUFFMAN, 1, rp.LEAN_MAX_CELLS, 4).leanEncode           # (batches never)
    # the pre-pass: a lane per tile up to 4,096 tiles
    assert rp.plan(KIND_HUFFMAN, 120, 150, 4096).prepass == 1 and rp.plan(KIND_HUFFMAN, 120, 150, 4097).prepass == 64
    # the roomy run: beside from 4,096 tiles unless the hint says none; skipped below 2,048 tiles when it says none
    assert rp.plan(KIND_HUFFMAN, 120, 150, 4096, roomy_seen=0).roomyForm == rp.ROOMY_BESIDE
    assert rp.plan(KIND_HUFFMAN, 120, 150, 4095, roomy_seen=0).roomyForm == rp.ROOMY_BEHIND
    assert rp.plan(KIND_HUFFMAN, 120, 150, 4096, roomy_seen=1).roomyForm == rp.ROOMY_BEHIND
    assert rp.plan(KIND_HUFFMAN, 120, 150, 2047, roomy_seen=1).roomyForm == rp.ROOMY_SKIPPED
    assert rp.plan(KIND_HUFFMAN, 120, 150, 2048, roomy_seen=1).roomyForm == rp.ROOMY_BEHIND
    assert rp.plan(KIND_HUFFMAN, 120, 150, 1000, roomy_seen=7).roomyForm == rp.ROOMY_BEHIND
    # the 2^28-cell limit
    with pytest.raises(ValueError):
        rp.plan(KIND_HUFFMAN, 1 << 14, 1 << 14)
    rp.plan(KIND_HUFFMAN, (1 << 14) - 1, 1 << 14)


def test_roomy_budget_matches_the_roomy_test_restatement():
    """tests/test_gpu_roomy.py decides which tiles the pre-pass lists from its own statement of the fast run's budget"""
    from test_gpu_roomy import _fast_lds_m32
    for r, c in rp.sweep():
        p = rp.plan(KIND_HUFFMAN, r, c)
        assert p.fastM32 == _fast_lds_m32(r * c) == _lds_m32(r, c), (r, c)
        roomy = min(98304, (2 * r * c + 1024 + 31) & ~31)
        assert p.ldsM32Roomy == (roomy if roomy > p.fastM32 else 0), (r, c)
