"""The library's preprocessor and environment switches are a fixed list.

Every GF_* name that a conditional directive (#if, #ifdef, #ifndef, #elif) of the library's sources tests, and every GF_*
variable they read with getenv, must be one of SWITCHES below.  A new switch is added here on purpose, with its reason;
an alternative that was measured and not kept is taken out of the sources, and out of this list, once its numbers are
recorded in DESIGN.md / profiles/HISTORY.md."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCHES = {
    # build flavours of gridfour_amd/build.py
    "GF_DIAG": "the diagnostic library: cycle stamps, phase ablation, gf_internal_* hooks",
    "GF_DIAG_SPLIT": "environment, diagnostic library only: the three-kernel encode form whose packer stamps tools/ read",
    "GF_DEC_VARIANT": "the legacy decoder's 512- and 1024-thread builds: their launchers renamed _t512 / _t1024",
    "GF_DEC_THREADS": "workgroup size of a legacy decoder build",
    "GF_DEC_MAXQ": "subsequences per chain of a legacy decoder build",
    "GF_CD_VARIANT": "the canonical decoder's 512-thread build: its launcher and LDS sizes renamed _t512",
    "GF_CD_THREADS": "workgroup size of a canonical decoder build",
    "GF_ENC_VARIANT": "the legacy encoder's 1024-thread build for the one-tile-per-call path",
    "GF_ENC_THREADS": "workgroup size of a legacy encoder build",
    # layout / host
    "GF_ENC_HIST_SEPARATE": "the reduced histograms as an array of their own: the diagnostic dump's layout",
    "GF_ENC_LAYOUT_FULL": "that layout outside the diagnostic build: tests/csrc/host_harness.cpp",
    "GF_HOST_HAS_CRC32_INSN": "defined by gvrs_api_records.hip on x86-64 hosts: CRC-32C by the SSE4.2 instruction",
    # numeric tunables: #ifndef X / #define X value, the sweep in the comment beside it
    "GF_ENC_PACK_WGS": "workgroups per CU of the Huffman packer",
    "GF_ENC_HIST_R_A": "histogram replicas of the encoder's phase-A kernel",
    "GF_ENC_A_WGS": "workgroups per CU of the encoder's phase-A kernel",
    "GF_CN_AB_WGS": "workgroups per CU of the canonical encoder's one-kernel form",
    "GF_CN_PACK_WGS": "workgroups per CU of the canonical packer",
    "GF_CN_A_WGS": "workgroups per CU of the canonical encoder's phase-A kernel",
    "GF_CN_TREES_WAVES": "waves per workgroup of the canonical code-length kernel",
    "GF_DEC_WGS": "workgroups per CU of the legacy decoder",
    "GF_DEC_MIN_UNIT": "bits of a subsequence of the fast Huffman pass, at least",
    "GF_DEC_EARLY_TXT": "how early the decoder fetches the packed text",
    "GF_LSOP_PREDICT_WGS": "workgroups per CU of the LSOP12 predictor",
    "GF_LSOP_PREDICT16_WGS": "workgroups per CU of the 16-bit LSOP12 predictor",
    "GF_LSOP_PACK2_WGS": "workgroups per CU of the LSOP12 packer",
    "GF_LSOP_HR16": "histogram replicas of the 16-bit LSOP12 predictor",
    "GF_LSOP_UNPACK_WAVES": "waves per SIMD the LSOP12 unpacker's register budget is cut for",
    "GF_PREPASS_ONE_LANE_MAX": "batch size up to which the Huffman tree pre-pass gives a tile a wave",
    "GF_CANON_PREPASS_ONE_LANE_MAX": "the same bound for the canonical pre-pass",
    "GF_CANON_T512_MIN_CELLS": "tile cells from which the canonical decoder may take its 512-thread build",
    # stress builds: a rare but correct path forced, or occupancy measured
    "GF_CN_FORCE_PM": "every canonical code table through the package-merge (tools/pm_lock_stress.py)",
    "GF_PT_FORCE_EXACT": "every tree of the decoder's pre-pass through the exact walk",
    "GF_DEC_POOL_FORCE_OVERFLOW": "the decoder's fall-back behind a symbol pool that overflowed",
    "GF_DEC_LDS_PAD_ENV": "occupancy sweep build: reads GF_DEC_LDS_PAD and GF_DEC_FORCE_THREADS (tools/occupancy_sweep.sh)",
    "GF_DEC_LDS_PAD": "environment, GF_DEC_LDS_PAD_ENV builds only: unused dynamic LDS per decoder workgroup",
    "GF_DEC_FORCE_THREADS": "environment, GF_DEC_LDS_PAD_ENV builds only: the decoder build to launch",
}

_DIRECTIVE = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$")
_NAME = re.compile(r"\bGF_[A-Z0-9_]+\b")
_GETENV = re.compile(r"\bgetenv\s*\(\s*\"(GF_[A-Z0-9_]+)\"")


def _sources():
    files = glob.glob(os.path.join(ROOT, "gridfour_amd", "csrc", "*.hip"))
    files += glob.glob(os.path.join(ROOT, "gridfour_amd", "csrc", "*.h"))
    for d in ("gridfour_amd/host", "include"):
        for base, _, names in os.walk(os.path.join(ROOT, d)):
            files += [os.path.join(base, n) for n in names]
    return sorted(files)


def switches_in(text):
    """GF_* names tested by conditional directives (comments aside) and GF_* variables read with getenv."""
    found = set(_GETENV.findall(text))
    for line in text.splitlines():
        m = _DIRECTIVE.match(line)
        if m:
            cond = re.sub(r"/\*.*?\*/", " ", m.group(1)).split("//")[0]
            found.update(_NAME.findall(cond))
    return found


def test_switch_scan_sees_every_form():
    text = ('#ifdef GF_A\n#ifndef GF_B  // GF_NOT_THIS\n#if defined(GF_C) && GF_D > 1\n#elif !defined( GF_E )\n'
            '#  if GF_F\nint x = GF_NOT_A_DIRECTIVE;\nconst char *e = getenv("GF_G");\n')
    assert switches_in(text) == {"GF_A", "GF_B", "GF_C", "GF_D", "GF_E", "GF_F", "GF_G"}


def test_build_switches_are_the_listed_ones():
    files = _sources()
    assert any(f.endswith("gvrs_decode.hip") for f in files), files
    found = {}
    for f in files:
        with open(f, encoding="utf-8", errors="replace") as fh:
            for name in switches_in(fh.read()):
                found.setdefault(name, []).append(os.path.relpath(f, ROOT))
    unlisted = {n: found[n] for n in sorted(set(found) - set(SWITCHES))}
    assert not unlisted, "switches not in SWITCHES (add one on purpose, with its reason): %s" % unlisted
    gone = sorted(set(SWITCHES) - set(found))
    assert not gone, "SWITCHES lists names the sources no longer test: %s" % gone
