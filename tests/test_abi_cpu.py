"""The C ABI is written down three times - the headers under include/, the table d2s.lib.ABI, the definitions in csrc/*.hip - and this
is the one test that ties them together: per header the declared names are the pinned ones and the table's; every name is declared once,
bound once and defined once; every entry's return type and parameters, parsed from its declaration, are what load() bound, one for one;
no source copies a prototype by hand, and each source includes the header of whatever it defines or calls, so the compiler compares
declaration and definition.  A new entry costs one declaration, one row under its header's key in d2s/lib.py and one name below."""
import ctypes
import os
import re

import pytest

from d2s import lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include")
CSRC = os.path.join(REPO, "dense2sparse-vit_amd", "csrc")

CORE = "d2s_hip.h"
CORE_ENTRIES = 120
# every other header, in the order they were added, with the names it declares, in declaration order
PINNED = {
    "d2s_hip_ext.h": ["d2s_attn_keyw_fwd_bf16", "d2s_tome_match_bf16"],
    "d2s_hip_squeeze.h": ["d2s_squeeze_match", "d2s_gather_squeeze_fwd", "d2s_gather_squeeze_bwd"],
    "d2s_hip_ats.h": ["d2s_ats_select"],
    "d2s_hip_ragged_train.h": ["d2s_attn_varlen_fwd_lse_f32", "d2s_attn_varlen_bwd_f32", "d2s_ragged_repack_bwd", "d2s_ragged_cls_scatter"],
    "d2s_hip_ragged_threshold.h": ["d2s_half_mean_concat_varlen_bwd", "d2s_ragged_mask_loss_fwd", "d2s_ragged_mask_loss_bwd",
                                   "d2s_ragged_teacher_rows"],
    "d2s_hip_avit.h": ["d2s_avit_halt", "d2s_avit_halt_bwd", "d2s_avit_penalty_fwd", "d2s_avit_penalty_bwd"],
    "d2s_hip_evo.h": ["d2s_evo_select", "d2s_evo_scatter_fwd", "d2s_evo_scatter_bwd", "d2s_evo_gather_bwd"],
    "d2s_hip_gemm_plan.h": ["d2s_gemm_f32_plan"],
    "d2s_hip_ragged_bf16.h": ["d2s_attn_varlen_fwd_lse_bf16", "d2s_attn_varlen_bwd_bf16"],
    "d2s_hip_ltp.h": ["d2s_ltp_score_workspace_bytes", "d2s_ltp_score_f32", "d2s_ltp_select", "d2s_ltp_soft_mask_fwd",
                      "d2s_ltp_soft_mask_bwd"],
    "d2s_hip_tome_train_bf16.h": ["d2s_attn_keyw_bwd_bf16", "d2s_tome_merge_bwd_bf16out"],
    "d2s_hip_ragged_stage_bf16.h": ["d2s_ragged_repack_bwd_bf16out", "d2s_avit_halt_repack_bwd_bf16out"],
    "d2s_hip_ltp_bf16.h": ["d2s_ltp_score_bf16_workspace_bytes", "d2s_ltp_score_bf16"],
    "d2s_hip_graph_rank.h": ["d2s_graph_rank_f32"],
    "d2s_hip_sim_prune.h": ["d2s_key_metric_f32", "d2s_sim_prune_f32"],
}
HEADERS = [CORE] + list(PINNED)
DIAGNOSTIC = {"d2s_debug_read_attn_stamps", "d2s_debug_read_stamps", "d2s_debug_read_stamps_f32"}      # defined, declared nowhere

RETURNS = {"int": lib.I, "size_t": lib.Z, "long": lib.L}
VALUES = {"int": lib.I, "long": lib.L, "float": lib.F, "size_t": lib.Z, "unsigned long long": ctypes.c_ulonglong}


def code(path):
    """a C / HIP file without its comments"""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def declarations(header):
    """[(name, return type, [parameter, ...])] of one header, in declaration order"""
    found = re.findall(r"^(int|size_t|long) (d2s_\w+)\((.*?)\);", code(os.path.join(INCLUDE, header)), flags=re.M | re.S)
    return [(name, ret, [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]) for ret, name, params in found]


def kind(param):
    """the ctypes type of one declared parameter: anything with a `*` and a stream are pointers, a value goes by its type"""
    if "*" in param or param.startswith("d2s_stream_t "):
        return lib.P
    return VALUES[param.rsplit(" ", 1)[0]]


def occurrences(path):
    """every `d2s_name(` of a source outside comments -> [(name, 'definition' | 'prototype' | 'use')]"""
    text, out = code(path), []
    for m in re.finditer(r"\b(d2s_\w+)\s*\(", text):
        end, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(text[end], 0)
            end += 1
        typed = re.search(r"\b(?:int|size_t|long)\s*$", text[:m.start()]) is not None
        after = text[end:].lstrip()[:1]
        out.append((m.group(1), "definition" if typed and after == "{" else "prototype" if typed and after == ";" else "use"))
    return out


def reachable(path, seen=None):
    """the quoted includes of a file, followed through csrc/ and include/"""
    seen = set() if seen is None else seen
    for inc in re.findall(r'^#include "([^"]+)"', open(path).read(), flags=re.M):
        if inc not in seen:
            seen.add(inc)
            reachable(next(p for p in (os.path.join(CSRC, inc), os.path.join(INCLUDE, inc)) if os.path.exists(p)), seen)
    return seen


SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
HEADER_OF = {name: header for header in HEADERS for name, _, _ in declarations(header)}


def test_the_table_has_one_key_per_header_in_order_and_nothing_else_is_in_include():
    assert list(lib.ABI) == HEADERS and sorted(os.listdir(INCLUDE)) == sorted(HEADERS)


@pytest.mark.parametrize("header", HEADERS)
def test_header_pinned_names_and_table_agree(header):
    text = open(os.path.join(INCLUDE, header)).read()
    declared = [name for name, _, _ in declarations(header)]
    if header == CORE:
        assert len(declared) == CORE_ENTRIES
    else:
        assert declared == PINNED[header] and '#include "d2s_hip.h"' in text
    assert sorted(declared) == lib.symbols(header) == sorted(lib.ABI[header])
    # the style rule: every `d2s_...(` outside comments is one declaration, `int|size_t|long d2s_...(` at the start of a line
    assert re.findall(r"\b(d2s_\w+)\s*\(", code(os.path.join(INCLUDE, header))) == declared


def test_every_name_is_declared_once_and_bound_once():
    declared = [name for header in HEADERS for name, _, _ in declarations(header)]
    bound = [name for header in lib.ABI for name in lib.ABI[header]]
    assert len(declared) == len(set(declared)) == CORE_ENTRIES + sum(len(v) for v in PINNED.values()) == 159
    assert len(bound) == len(set(bound)) and sorted(bound) == sorted(declared) == lib.symbols()
    for name in declared:
        assert lib.signature(name) is lib.ABI[HEADER_OF[name]][name], name


@pytest.mark.parametrize("header", HEADERS)
def test_every_declaration_equals_its_ctypes_row_and_what_load_bound(header):
    handle = lib.load()
    for name, ret, params in declarations(header):
        fn = getattr(handle, name)                                   # load() resolved it, and call() / query() reach it
        assert lib._fn(name) is fn and callable(fn), name
        res, args = lib.signature(name)
        stream = bool(params) and params[-1] == "d2s_stream_t stream"
        kinds = [kind(p) for p in params]
        assert res is RETURNS[ret] and fn.restype is res, name
        assert (args is None) == (not params), name                 # `(void)` is the row without argtypes
        assert kinds == list(args or []) + [lib.P] * stream, name    # the row, one for one, and the stream exactly where it is declared
        assert fn.argtypes == kinds, name
        assert stream == (res is lib.I and args is not None), name  # the rule beside the table: what launches takes the stream


def test_every_entry_is_defined_once_and_no_source_copies_a_prototype():
    defined = []
    for src in SOURCES:
        found = occurrences(os.path.join(CSRC, src))
        assert [name for name, what in found if what == "prototype"] == [], src
        defined += [name for name, what in found if what == "definition"]
    assert len(defined) == len(set(defined)) and set(defined) == set(HEADER_OF) | DIAGNOSTIC
    for helper in ("d2s_common.h", "gemm_common.h"):
        assert all(what == "use" or name not in HEADER_OF for name, what in occurrences(os.path.join(CSRC, helper))), helper


@pytest.mark.parametrize("src", SOURCES)
def test_a_source_includes_the_header_of_what_it_defines_or_calls(src):
    path = os.path.join(CSRC, src)
    names = {name for name, _ in occurrences(path) if name in HEADER_OF}
    assert names, src                                                # every source defines at least one entry
    assert {HEADER_OF[name] for name in names} <= reachable(path), src


def test_the_error_codes_are_defined_once():
    common = open(os.path.join(CSRC, "d2s_common.h")).read()
    assert '#include "d2s_hip.h"' in common
    defines = [f for d, fs in ((CSRC, os.listdir(CSRC)), (INCLUDE, HEADERS)) for f in fs
               if os.path.isfile(os.path.join(d, f)) and re.search(r"^#define D2S_(?:OK|ERR_\w+)\b", open(os.path.join(d, f)).read(), flags=re.M)]
    assert defines == [CORE]
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "-I../../include" in makefile and "$(wildcard ../../include/*.h)" in makefile
