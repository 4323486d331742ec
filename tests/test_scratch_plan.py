"""The scratch plan (gf_internal_scratch_plan, gvrs_api_route.hip), on the CPU: what encodeBatchDev, decodeBatchDev and the LSOP12
launch sites ask of the context's workspace, trees and packRecs is what gf_context_reserve allocates at the most -- the promise of
include/gvrs_hip_codec.h that a _dev call after gf_context_reserve never allocates -- and every part lies inside its buffer."""
import route_plan as rp
import scratch_plan as sp

TILE_COUNTS = (1, 2, 63, 64, 65, 4095, 4096, 12960)


def test_reserve_covers_every_plan_and_parts_lie_inside():
    n = 0
    for r, c in rp.sweep():
        for nt in TILE_COUNTS:
            res = sp.reserve(r, c, nt)
            for kind, lean, via_fast in sp.variants():
                p = sp.plan(kind, r, c, nt, lean, via_fast)
                for buf, have in zip(sp.BUFFERS, res):
                    assert have >= getattr(p, buf), (buf, kind, r, c, nt, lean, via_fast)
                for buf, parts in sp.PARTS.items():
                    for name in parts:
                        part = getattr(p, name)
                        assert part.at + part.bytes <= getattr(p, buf), (name, kind, r, c, nt, lean, via_fast)
                assert p.wsStride * min(max(nt, 1), 2048) == p.workspace, (kind, r, c, nt)
                n += 1
    assert n > 80000


def test_parts_are_those_of_the_kind():
    """each kind has its parts, one behind the other, and no other kind's"""
    for nt in TILE_COUNTS:
        p = sp.plan(rp.KIND_HUFFMAN, 120, 150, nt)
        assert p.leaf.at == 0 and p.spare.at == p.leaf.bytes and p.spare.bytes == 16 and p.roomy.at == p.spare.at + 16
        assert p.leaf.bytes == nt * 648 * 4 and p.roomy.bytes == nt * 4 and p.lengths.bytes == p.lsop0.bytes == p.hist.bytes == 0
        assert p.sel.at == 0 and p.stats.at == p.sel.bytes and p.plane.at >= p.stats.at + p.stats.bytes and p.plane.at % 256 == 0
        assert p.plane.bytes == nt * p.planeStride and p.planeStride == 120 * 150 + (-120 * 150) % 16
        lean = sp.plan(rp.KIND_HUFFMAN, 120, 150, nt, lean=1)
        assert lean.plane.bytes == 0 and lean.planeStride == 0 and lean.packRecs == p.packRecs
        slow, fast = sp.plan(rp.KIND_CANON, 120, 150, nt), sp.plan(rp.KIND_CANON, 120, 150, nt, via_fast=1)
        assert slow.lengths.bytes == nt * 76 * 4 and slow.slack.at == slow.lengths.bytes and fast.trees == slow.trees + 4096
        assert slow.workspace == 0 and slow.leaf.bytes == 0 and slow.packRecs == p.packRecs
        d = sp.plan(sp.KIND_LSOP_DEC, 120, 150, nt)
        assert d.lsop0.at == 0 and d.lsop1.at == d.lsop0.bytes == d.lsop1.bytes == nt * 76 * 4 and d.packRecs == 0
        assert d.workspace == p.workspace
        e = sp.plan(sp.KIND_LSOP_ENC, 120, 150, nt)
        assert e.hist.at == 0 and 0 < e.hist.bytes < e.packRecs and e.trees == 0 and e.workspace == 0
        m = sp.plan(rp.KIND_RAW_M32, 120, 150, nt)
        assert m.workspace == p.workspace and m.trees == 0
