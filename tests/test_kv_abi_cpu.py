"""The paged-KV entry points of the C ABI reject what they always rejected, with the same code and the same fq_last_error() text.

Validation returns before any HIP call, so this runs without a GPU. Every case below is a REJECTED call: a table of argument sets per
entry point (one fault each, plus pairs of faults that pin which check wins), and the (code, message) each one must produce. The
expected pairs and the workspace sizes were recorded from the library as it stood before the entry points were folded onto shared
validation helpers (version 120); `python tests/test_kv_abi_cpu.py` prints both tables for whatever library is loaded (FQHIP_LIB).
"""
import itertools

import pytest

P = 4096       # a non-NULL, 16-byte aligned address (never dereferenced: every call here fails validation first)
ODD = 4104     # a misaligned one

_CACHE = [("kv_data", P), ("kv_param", P), ("kv_indptr", P), ("kv_indices", P), ("last_page_offset", P)]
_GEOM = [("num_layers", 2), ("layer_idx", 1)]
_WS = [("seq_hint", 0), ("workspace", None), ("workspace_bytes", 0)]
_OQ = [("o", P), ("q", P), ("q_trans", None), ("transpose_out", 0)]
_NEW = [("k_new", P), ("v_new", P), ("k_trans_image", None), ("src_heads", 8)]
_APPEND = _CACHE + [("k", P), ("v", P), ("k_param", P), ("v_param", P), ("seqlen_indptr", None), ("tokens", 2)] + _GEOM + [
    ("num_heads", 8), ("page_size", 16), ("head_dim", 128), ("batch_size", 2), ("group_size", 1), ("stream", None)]
_PLAIN_EX = _OQ + _CACHE + _GEOM + [("num_heads", 8), ("page_size", 16), ("head_dim", 128), ("batch_size", 2), ("stream", None)]
_PLAIN = [("o", P), ("q", P)] + _PLAIN_EX[4:]
_DECODE_APPEND = _OQ + _NEW + _CACHE + _GEOM + [("num_kv_heads", 8), ("q_group", 4), ("page_size", 16), ("head_dim", 128),
                                                 ("batch_size", 2)] + _WS[:1] + [("read_one_copy", 0)] + _WS[1:] + [("stream", None)]

# entry point -> its arguments in order, with values that pass validation (a case replaces some of them)
ENTRIES = {
    "fq_kv_append_i4": _APPEND,
    "fq_kv_append_f16": _APPEND,
    "fq_kv_quant_append_i4": [("k", P), ("v", P), ("trans", None), ("tokens", 2), ("src_heads", 8), ("head_dim", 128), ("clip", None),
                              ("flags", 0)] + _CACHE + _GEOM + [("num_heads", 8), ("page_size", 16), ("batch_size", 2), ("group_size", 1),
                                                                 ("stream", None)],
    "fq_kv_batch_decode_i4": _PLAIN,
    "fq_kv_batch_decode_f16": _PLAIN,
    "fq_kv_batch_decode_i4_ex": _PLAIN_EX,
    "fq_kv_batch_decode_f16_ex": _PLAIN_EX,
    "fq_kv_batch_decode_split": [("fp16_cache", 0)] + _OQ + _CACHE + _GEOM + [("num_heads", 8), ("page_size", 16), ("head_dim", 128),
                                                                              ("batch_size", 2)] + _WS + [("stream", None)],
    "fq_kv_batch_decode_gqa": [("fp16_cache", 0)] + _OQ + _CACHE + _GEOM + [("num_kv_heads", 8), ("q_group", 4), ("page_size", 16),
                                                                            ("head_dim", 128), ("batch_size", 2)] + _WS + [("stream", None)],
    "fq_kv_batch_decode_copies": [("fp16_cache", 0)] + _OQ + _CACHE + _GEOM + [("num_heads", 8), ("copies", 4), ("page_size", 16),
                                                                               ("head_dim", 128), ("batch_size", 2)] + _WS + [("stream", None)],
    "fq_kv_decode_append_i4": _DECODE_APPEND,
    "fq_kv_decode_append_rope_i4": _DECODE_APPEND + [("cos", P), ("sin", P)],
    "fq_kv_decode_append_had_i4": [a for a in _DECODE_APPEND if a[0] not in ("q_trans", "k_trans_image")] + [("had_scale", 0.125)],
    "fq_kv_batch_extend": [("fp16_cache", 0)] + _OQ + _CACHE + _GEOM + [("num_cache_heads", 8), ("q_group", 4), ("copies", 1), ("q_len", 3),
                                                                        ("page_size", 16), ("head_dim", 128), ("batch_size", 2)] + _WS + [
                                                                            ("stream", None)],
    "fq_kv_chunk_extend": [("fp16_cache", 0)] + _OQ + _CACHE + _GEOM + [("num_cache_heads", 8), ("q_group", 4), ("copies", 1), ("q_len", 3),
                                                                        ("page_size", 16), ("head_dim", 128), ("batch_size", 2), ("stream", None)],
    "fq_prefill_attention_f16": [("o", P), ("q", P), ("q_trans", None), ("k", P), ("v", P), ("seq_start", None), ("seq_len", None),
                                 ("batch_size", 2), ("seq", 130), ("q_heads", 8), ("kv_heads", 2), ("head_dim", 128), ("stream", None)],
}

_POINTERS = {"kv_data", "kv_param", "kv_indptr", "kv_indices", "last_page_offset", "k", "v", "k_param", "v_param", "seqlen_indptr", "trans",
             "o", "q", "q_trans", "k_new", "v_new", "k_trans_image", "workspace", "cos", "sin", "seq_start", "seq_len"}
_OPTIONAL = {"seqlen_indptr", "trans", "q_trans", "k_trans_image", "workspace", "seq_start", "seq_len", "cos", "sin"}
_NO_PARAMS = {"fq_kv_batch_decode_f16", "fq_kv_batch_decode_f16_ex"}     # fp16 pages: kv_param may be NULL
# the pointers each entry point wants on a 16-byte boundary (the others it only hands on)
_ALIGNED = {"fq_kv_append": ["kv_data", "k", "v"], "fq_kv_quant_append": ["k", "v", "trans", "kv_data"],
            "fq_kv_batch_decode": ["kv_data", "q_trans", "workspace"], "fq_kv_batch_extend": ["kv_data", "q_trans", "workspace"],
            "fq_kv_decode_append": ["kv_data", "q_trans", "workspace", "k_new", "v_new", "k_trans_image", "cos", "sin"],
            "fq_kv_chunk_extend": ["o", "q", "kv_data", "q_trans"]}
# a geometry whose decode launch splits: 1 request x 2 heads x head_dim 128 at 512 cached rows; the workspace is one byte short
_SPLITS = dict(batch_size=1, head_dim=128, seq_hint=512, workspace=P)


def _heads_arg(names):
    return next(n for n in ("num_heads", "num_kv_heads", "num_cache_heads") if n in names)


def _workspace_need(lib, entry, args):
    """what the exported sizing function says for the launch `args` describes (those functions are pinned below)"""
    if entry == "fq_kv_batch_decode_split":
        return lib.fq_kv_decode_workspace_bytes(args["batch_size"], args["num_heads"], args["head_dim"])
    if entry == "fq_kv_batch_decode_copies":
        return lib.fq_kv_decode_workspace_bytes_gqa(args["batch_size"], args["num_heads"] // args["copies"], args["copies"], args["head_dim"])
    if entry == "fq_kv_batch_extend":
        q_heads = args["num_cache_heads"] // args["copies"] * args["q_group"]
        return lib.fq_kv_extend_workspace_bytes(args["batch_size"], q_heads, args["q_len"], args["head_dim"])
    share = args["q_group"]
    if args.get("read_one_copy") and share == 1:
        share = args["num_kv_heads"] // args["src_heads"]
    return lib.fq_kv_decode_workspace_bytes_gqa(args["batch_size"], args["num_kv_heads"] * args["q_group"] // share, share, args["head_dim"])


def cases(entry):
    """[(case id, {argument: value})]: the rejected calls of one entry point. A value of "short" for workspace_bytes stands for one byte
    less than the launch needs."""
    names = [n for n, _ in ENTRIES[entry]]
    out = []

    def add(cid, **changes):
        assert all(k in names for k in changes), (entry, cid)
        out.append((cid, changes))

    if entry == "fq_prefill_attention_f16":
        add("head_dim_64", head_dim=64)
        add("head_dim_96", head_dim=96)
        add("batch_0", batch_size=0)
        add("seq_0", seq=0)
        add("heads_not_multiple", q_heads=7)
        add("seq_start_alone", seq_start=P)
        add("seq_len_alone", seq_len=P)
        for n in ("o", "q", "k", "v"):
            add(f"null_{n}", **{n: None})
        for n in ("o", "q", "q_trans", "k", "v", "seq_start", "seq_len"):
            add(f"odd_{n}", **{n: ODD})
        add("two_odd_v_and_head_dim_64", v=ODD, head_dim=64)
        add("two_head_dim_64_and_batch_0", head_dim=64, batch_size=0)
        add("two_seq_start_alone_and_null_o", seq_start=P, o=None)
        return out

    heads = _heads_arg(names)
    required = [n for n in names if n in _POINTERS and n not in _OPTIONAL]
    first = required[0]
    add("bad_layer", layer_idx=2)
    add("negative_layer", layer_idx=-1)
    add("batch_0", batch_size=0)
    add("head_dim_96", head_dim=96)
    add("page_size_0", page_size=0)
    for n in required:
        if n == "kv_param" and entry in _NO_PARAMS:
            add("null_kv_param", kv_param=None, kv_data=ODD)               # (fp16 pages carry no params: it passes the NULL check, and the
        else:                                                               #  misaligned pointer, which is checked next, stops the call)
            add(f"null_{n}", **{n: None})
        if n == "kv_param" and "fp16_cache" in names:
            add("null_kv_param_fp16_cache", kv_param=None, fp16_cache=1, q_trans=ODD)
    aligned = [n for n in next(v for k, v in _ALIGNED.items() if entry.startswith(k)) if n in names]
    for n in aligned:
        add(f"odd_{n}", **{n: ODD})
    add("two_bad_layer_and_null", layer_idx=2, **{first: None})
    add("two_head_dim_96_and_batch_0", head_dim=96, batch_size=0)
    add("two_null_and_odd", **{required[-1]: None, "kv_data": ODD})
    add("two_odd_pointers", **{n: ODD for n in aligned[:2]})

    if "q_group" in names:
        add("q_group_0", q_group=0)
        add("q_group_65", q_group=65)
        add("two_q_group_65_and_null", q_group=65, **{first: None})
        add("two_q_group_0_and_bad_layer", q_group=0, layer_idx=2)
    if "copies" in names:
        add("copies_9", copies=9, **({"q_group": 9} if "q_group" in names else {}))
        add("copies_0", copies=0)
        add("copies_not_dividing_heads", copies=3, **({"q_group": 3} if "q_group" in names else {}))
        add("two_copies_9_and_null", copies=9, **{first: None})
    if "q_group" in names and "copies" in names:
        add("q_group_not_multiple_of_copies", q_group=4, copies=8)
        add("q_len_0", q_len=0)
        add("two_q_len_0_and_bad_layer", q_len=0, layer_idx=2)
        add("head_dim_64", head_dim=64)
        add("two_head_dim_64_and_copies_9", head_dim=64, copies=9)
        add("two_head_dim_64_and_null", head_dim=64, o=None)
    if entry == "fq_kv_chunk_extend":
        add("q_group_3", q_group=3)
        add("two_q_group_3_and_null", q_group=3, o=None)
        add("two_q_group_3_and_head_dim_64", q_group=3, head_dim=64)
        add("too_many_rows", q_len=0x7FFFFFFF, q_group=8)
        add("two_too_many_rows_and_odd_q", q_len=0x7FFFFFFF, q_group=8, q=ODD)
    if entry.startswith("fq_kv_decode_append"):
        add("page_size_8", page_size=8)
        add("head_dim_64", head_dim=64)
        add("src_heads_0", src_heads=0)
        add("src_heads_not_dividing", src_heads=3)
        add("src_group_over_8", num_kv_heads=16, src_heads=1)
        add("two_page_size_8_and_q_group_65", page_size=8, q_group=65)
        add("two_page_size_8_and_src_heads_0", page_size=8, src_heads=0)
        add("two_src_heads_0_and_null", src_heads=0, k_new=None)
    if entry == "fq_kv_decode_append_rope_i4":
        add("cos_without_sin", sin=None)
        add("sin_without_cos", cos=None)
        add("two_cos_without_sin_and_odd_workspace", sin=None, workspace=ODD)
        add("two_cos_without_sin_and_odd_cos", sin=None, cos=ODD)
        add("two_cos_without_sin_and_null", sin=None, v_new=None)
        add("two_odd_sin_and_short_workspace", sin=ODD, workspace_bytes="short", num_kv_heads=2, q_group=1, src_heads=2, **_SPLITS)
    if entry.startswith("fq_kv_append"):
        add("tokens_negative", tokens=-1)
        add("tokens_not_batch", tokens=3)
        add("group_size_0", group_size=0)
        add("group_size_not_dividing", group_size=3)
        add("two_group_size_0_and_tokens_negative", group_size=0, tokens=-1)
        add("two_tokens_not_batch_and_null", tokens=3, k=None)
        add("two_head_dim_96_and_group_size_0", head_dim=96, group_size=0)
    if entry == "fq_kv_quant_append_i4":
        add("unknown_flags", flags=2)
        add("tokens_not_multiple_of_batch", tokens=3)
        add("tokens_negative", tokens=-2)
        add("src_heads_0", src_heads=0)
        add("group_size_9", group_size=9, src_heads=1, num_heads=9)
        add("heads_not_src_times_group", group_size=2)
        add("two_unknown_flags_and_tokens", flags=2, tokens=3)
        add("two_tokens_and_group", tokens=3, group_size=2)
        add("two_group_and_null", group_size=2, k=None)
    if "workspace_bytes" in names:
        small = {heads: 2, **_SPLITS}
        if "q_group" in names:
            small["q_group"] = 1
        if "copies" in names:
            small["copies"] = 1
        if "src_heads" in names:
            small["src_heads"] = 2
        if "q_len" in names:
            small["q_len"] = 1
        add("workspace_one_short", workspace_bytes="short", **small)
        add("workspace_bytes_0", workspace_bytes=0, **small)
        add("two_workspace_short_and_odd_workspace", workspace_bytes="short", **{**small, "workspace": ODD})
        add("two_workspace_short_and_null", workspace_bytes="short", **{**small, "q": None})
        if "fp16_cache" in names:
            add("workspace_one_short_fp16_cache", workspace_bytes="short", fp16_cache=1, kv_param=None, **small)
    if entry == "fq_kv_batch_decode_gqa":      # the merged workgroups: 4 requests x 8 KV heads x 4 query heads split 8 ways at 2048 rows
        add("workspace_one_short_merged", workspace_bytes="short", batch_size=4, seq_hint=2048, workspace=P)
    if entry == "fq_kv_batch_decode_copies":
        add("workspace_one_short_copies_4", workspace_bytes="short", batch_size=1, seq_hint=1024, workspace=P)
    if entry.startswith("fq_kv_decode_append"):
        add("workspace_one_short_read_one_copy", workspace_bytes="short", batch_size=1, num_kv_heads=8, src_heads=2, q_group=1, read_one_copy=1,
            seq_hint=1024, workspace=P)
    return out


def call(lib, entry, changes):
    args = dict(ENTRIES[entry])
    args.update(changes)
    if args.get("workspace_bytes") == "short":
        need = _workspace_need(lib, entry, args)
        assert need > 0, (entry, changes)
        args["workspace_bytes"] = need - 1
    code = getattr(lib, entry)(*[args[n] for n, _ in ENTRIES[entry]])
    return code, lib.fq_last_error().decode()


_BATCH, _HEADS, _GROUP, _HD, _QLEN = (1, 4, 16, 129), (2, 8, 32), (1, 2, 4, 8), (64, 128), (1, 3)


def workspace_sizes(lib):
    return {
        "fq_kv_decode_workspace_bytes": [lib.fq_kv_decode_workspace_bytes(b, h, d) for b, h, d in itertools.product(_BATCH, _HEADS, _HD)],
        "fq_kv_decode_workspace_bytes_gqa": [lib.fq_kv_decode_workspace_bytes_gqa(b, h, g, d)
                                             for b, h, g, d in itertools.product(_BATCH, _HEADS, _GROUP, _HD)],
        "fq_kv_extend_workspace_bytes": [lib.fq_kv_extend_workspace_bytes(b, h, t, d) for b, h, t, d in itertools.product(_BATCH, _HEADS, _QLEN, _HD)],
    }


# ---- recorded from the library before the refactor (version 120) ----
WORKSPACE_SIZES = {'fq_kv_decode_workspace_bytes': [8464, 16656, 33824, 66592, 135296, 266368, 33824, 66592, 135296, 266368, 541184, 1065472, 135296, 266368, 541184,
                                  1065472, 0, 0, 0, 0, 0, 0, 0, 0],
 'fq_kv_decode_workspace_bytes_gqa': [8464, 16656, 16912, 33296, 33824, 66592, 67648, 133184, 33824, 66592, 67648, 133184, 135296, 266368, 270592,
                                      532736, 135296, 266368, 270592, 532736, 541184, 1065472, 0, 2130944, 33824, 66592, 67648, 133184, 135296,
                                      266368, 270592, 532736, 135296, 266368, 270592, 532736, 541184, 1065472, 0, 2130944, 541184, 1065472, 0,
                                      2130944, 0, 4261888, 0, 0, 135296, 266368, 270592, 532736, 541184, 1065472, 0, 2130944, 541184, 1065472, 0,
                                      2130944, 0, 4261888, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                      0, 0, 0, 0],
 'fq_kv_extend_workspace_bytes': [0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0,
                                  2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 2130432, 0, 0, 0, 0,
                                  0, 0, 0, 0, 0, 0, 0, 0]}

EXPECTED = {'fq_kv_append_i4': {'bad_layer': (-1, 'fq_kv_append_i4: bad cache geometry'),
                     'negative_layer': (-1, 'fq_kv_append_i4: bad cache geometry'),
                     'batch_0': (-1, 'fq_kv_append_i4: bad cache geometry'),
                     'head_dim_96': (-2, 'fq_kv_append_i4: head_dim=96 (64 or 128)'),
                     'page_size_0': (-1, 'fq_kv_append_i4: bad cache geometry'),
                     'null_kv_data': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'null_kv_param': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'null_kv_indptr': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'null_kv_indices': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'null_last_page_offset': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'null_k': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'null_v': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'null_k_param': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'null_v_param': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'odd_kv_data': (-1, 'fq_kv_append_i4: pointer argument 0 of {kv_data, k, v} is not 16-byte aligned'),
                     'odd_k': (-1, 'fq_kv_append_i4: pointer argument 1 of {kv_data, k, v} is not 16-byte aligned'),
                     'odd_v': (-1, 'fq_kv_append_i4: pointer argument 2 of {kv_data, k, v} is not 16-byte aligned'),
                     'two_bad_layer_and_null': (-1, 'fq_kv_append_i4: bad cache geometry'),
                     'two_head_dim_96_and_batch_0': (-1, 'fq_kv_append_i4: bad cache geometry'),
                     'two_null_and_odd': (-1, 'fq_kv_append_i4: NULL pointer'),
                     'two_odd_pointers': (-1, 'fq_kv_append_i4: pointer argument 0 of {kv_data, k, v} is not 16-byte aligned'),
                     'tokens_negative': (-1, 'fq_kv_append_i4: tokens < 0'),
                     'tokens_not_batch': (-1, 'fq_kv_append_i4: without seqlen_indptr every request appends one token (tokens == batch_size)'),
                     'group_size_0': (-1, 'fq_kv_append_i4: group_size=0 must divide num_heads=8'),
                     'group_size_not_dividing': (-1, 'fq_kv_append_i4: group_size=3 must divide num_heads=8'),
                     'two_group_size_0_and_tokens_negative': (-1, 'fq_kv_append_i4: group_size=0 must divide num_heads=8'),
                     'two_tokens_not_batch_and_null': (-1,
                                                       'fq_kv_append_i4: without seqlen_indptr every request appends one token (tokens == '
                                                       'batch_size)'),
                     'two_head_dim_96_and_group_size_0': (-2, 'fq_kv_append_i4: head_dim=96 (64 or 128)')},
 'fq_kv_append_f16': {'bad_layer': (-1, 'fq_kv_append_f16: bad cache geometry'),
                      'negative_layer': (-1, 'fq_kv_append_f16: bad cache geometry'),
                      'batch_0': (-1, 'fq_kv_append_f16: bad cache geometry'),
                      'head_dim_96': (-2, 'fq_kv_append_f16: head_dim=96 (64 or 128)'),
                      'page_size_0': (-1, 'fq_kv_append_f16: bad cache geometry'),
                      'null_kv_data': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'null_kv_param': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'null_kv_indptr': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'null_kv_indices': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'null_last_page_offset': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'null_k': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'null_v': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'null_k_param': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'null_v_param': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'odd_kv_data': (-1, 'fq_kv_append_f16: pointer argument 0 of {kv_data, k, v} is not 16-byte aligned'),
                      'odd_k': (-1, 'fq_kv_append_f16: pointer argument 1 of {kv_data, k, v} is not 16-byte aligned'),
                      'odd_v': (-1, 'fq_kv_append_f16: pointer argument 2 of {kv_data, k, v} is not 16-byte aligned'),
                      'two_bad_layer_and_null': (-1, 'fq_kv_append_f16: bad cache geometry'),
                      'two_head_dim_96_and_batch_0': (-1, 'fq_kv_append_f16: bad cache geometry'),
                      'two_null_and_odd': (-1, 'fq_kv_append_f16: NULL pointer'),
                      'two_odd_pointers': (-1, 'fq_kv_append_f16: pointer argument 0 of {kv_data, k, v} is not 16-byte aligned'),
                      'tokens_negative': (-1, 'fq_kv_append_f16: tokens < 0'),
                      'tokens_not_batch': (-1, 'fq_kv_append_f16: without seqlen_indptr every request appends one token (tokens == batch_size)'),
                      'group_size_0': (-1, 'fq_kv_append_f16: group_size=0 must divide num_heads=8'),
                      'group_size_not_dividing': (-1, 'fq_kv_append_f16: group_size=3 must divide num_heads=8'),
                      'two_group_size_0_and_tokens_negative': (-1, 'fq_kv_append_f16: group_size=0 must divide num_heads=8'),
                      'two_tokens_not_batch_and_null': (-1,
                                                        'fq_kv_append_f16: without seqlen_indptr every request appends one token (tokens == '
                                                        'batch_size)'),
                      'two_head_dim_96_and_group_size_0': (-2, 'fq_kv_append_f16: head_dim=96 (64 or 128)')},
 'fq_kv_quant_append_i4': {'bad_layer': (-1, 'fq_kv_quant_append_i4: bad cache geometry'),
                           'negative_layer': (-1, 'fq_kv_quant_append_i4: bad cache geometry'),
                           'batch_0': (-1, 'fq_kv_quant_append_i4: bad cache geometry'),
                           'head_dim_96': (-2, 'fq_kv_quant_append_i4: head_dim=96 (64 or 128)'),
                           'page_size_0': (-1, 'fq_kv_quant_append_i4: bad cache geometry'),
                           'null_k': (-1, 'fq_kv_quant_append_i4: NULL pointer'),
                           'null_v': (-1, 'fq_kv_quant_append_i4: NULL pointer'),
                           'null_kv_data': (-1, 'fq_kv_quant_append_i4: NULL pointer'),
                           'null_kv_param': (-1, 'fq_kv_quant_append_i4: NULL pointer'),
                           'null_kv_indptr': (-1, 'fq_kv_quant_append_i4: NULL pointer'),
                           'null_kv_indices': (-1, 'fq_kv_quant_append_i4: NULL pointer'),
                           'null_last_page_offset': (-1, 'fq_kv_quant_append_i4: NULL pointer'),
                           'odd_k': (-1, 'fq_kv_quant_append_i4: pointer argument 0 of {k, v, trans, kv_data} is not 16-byte aligned'),
                           'odd_v': (-1, 'fq_kv_quant_append_i4: pointer argument 1 of {k, v, trans, kv_data} is not 16-byte aligned'),
                           'odd_trans': (-1, 'fq_kv_quant_append_i4: pointer argument 2 of {k, v, trans, kv_data} is not 16-byte aligned'),
                           'odd_kv_data': (-1, 'fq_kv_quant_append_i4: pointer argument 3 of {k, v, trans, kv_data} is not 16-byte aligned'),
                           'two_bad_layer_and_null': (-1, 'fq_kv_quant_append_i4: bad cache geometry'),
                           'two_head_dim_96_and_batch_0': (-1, 'fq_kv_quant_append_i4: bad cache geometry'),
                           'two_null_and_odd': (-1, 'fq_kv_quant_append_i4: NULL pointer'),
                           'two_odd_pointers': (-1, 'fq_kv_quant_append_i4: pointer argument 0 of {k, v, trans, kv_data} is not 16-byte aligned'),
                           'unknown_flags': (-1, 'fq_kv_quant_append_i4: unknown flags 0x2'),
                           'tokens_not_multiple_of_batch': (-1, 'fq_kv_quant_append_i4: tokens=3 must be a multiple of batch_size=2'),
                           'tokens_negative': (-1, 'fq_kv_quant_append_i4: tokens=-2 must be a multiple of batch_size=2'),
                           'src_heads_0': (-1, 'fq_kv_quant_append_i4: tokens=2 must be a multiple of batch_size=2'),
                           'group_size_9': (-1, 'fq_kv_quant_append_i4: num_heads=9 must be src_heads=1 x group_size=9 (<= 8)'),
                           'heads_not_src_times_group': (-1, 'fq_kv_quant_append_i4: num_heads=8 must be src_heads=8 x group_size=2 (<= 8)'),
                           'two_unknown_flags_and_tokens': (-1, 'fq_kv_quant_append_i4: unknown flags 0x2'),
                           'two_tokens_and_group': (-1, 'fq_kv_quant_append_i4: tokens=3 must be a multiple of batch_size=2'),
                           'two_group_and_null': (-1, 'fq_kv_quant_append_i4: num_heads=8 must be src_heads=8 x group_size=2 (<= 8)')},
 'fq_kv_batch_decode_i4': {'bad_layer': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                           'negative_layer': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                           'batch_0': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                           'head_dim_96': (-2, 'fq_kv_batch_decode_i4: head_dim=96 (64 or 128)'),
                           'page_size_0': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                           'null_o': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                           'null_q': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                           'null_kv_data': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                           'null_kv_param': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                           'null_kv_indptr': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                           'null_kv_indices': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                           'null_last_page_offset': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                           'odd_kv_data': (-1, 'fq_kv_batch_decode_i4: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned'),
                           'two_bad_layer_and_null': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                           'two_head_dim_96_and_batch_0': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                           'two_null_and_odd': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                           'two_odd_pointers': (-1, 'fq_kv_batch_decode_i4: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned')},
 'fq_kv_batch_decode_f16': {'bad_layer': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                            'negative_layer': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                            'batch_0': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                            'head_dim_96': (-2, 'fq_kv_batch_decode_f16: head_dim=96 (64 or 128)'),
                            'page_size_0': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                            'null_o': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                            'null_q': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                            'null_kv_data': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                            'null_kv_param': (-1, 'fq_kv_batch_decode_f16: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned'),
                            'null_kv_indptr': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                            'null_kv_indices': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                            'null_last_page_offset': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                            'odd_kv_data': (-1, 'fq_kv_batch_decode_f16: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned'),
                            'two_bad_layer_and_null': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                            'two_head_dim_96_and_batch_0': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                            'two_null_and_odd': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                            'two_odd_pointers': (-1, 'fq_kv_batch_decode_f16: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned')},
 'fq_kv_batch_decode_i4_ex': {'bad_layer': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                              'negative_layer': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                              'batch_0': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                              'head_dim_96': (-2, 'fq_kv_batch_decode_i4: head_dim=96 (64 or 128)'),
                              'page_size_0': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                              'null_o': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                              'null_q': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                              'null_kv_data': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                              'null_kv_param': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                              'null_kv_indptr': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                              'null_kv_indices': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                              'null_last_page_offset': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                              'odd_kv_data': (-1, 'fq_kv_batch_decode_i4: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned'),
                              'odd_q_trans': (-1, 'fq_kv_batch_decode_i4: pointer argument 1 of {kv_data, q_trans} is not 16-byte aligned'),
                              'two_bad_layer_and_null': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                              'two_head_dim_96_and_batch_0': (-1, 'fq_kv_batch_decode_i4: bad cache geometry'),
                              'two_null_and_odd': (-1, 'fq_kv_batch_decode_i4: NULL pointer'),
                              'two_odd_pointers': (-1, 'fq_kv_batch_decode_i4: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned')},
 'fq_kv_batch_decode_f16_ex': {'bad_layer': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                               'negative_layer': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                               'batch_0': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                               'head_dim_96': (-2, 'fq_kv_batch_decode_f16: head_dim=96 (64 or 128)'),
                               'page_size_0': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                               'null_o': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                               'null_q': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                               'null_kv_data': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                               'null_kv_param': (-1, 'fq_kv_batch_decode_f16: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned'),
                               'null_kv_indptr': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                               'null_kv_indices': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                               'null_last_page_offset': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                               'odd_kv_data': (-1, 'fq_kv_batch_decode_f16: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned'),
                               'odd_q_trans': (-1, 'fq_kv_batch_decode_f16: pointer argument 1 of {kv_data, q_trans} is not 16-byte aligned'),
                               'two_bad_layer_and_null': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                               'two_head_dim_96_and_batch_0': (-1, 'fq_kv_batch_decode_f16: bad cache geometry'),
                               'two_null_and_odd': (-1, 'fq_kv_batch_decode_f16: NULL pointer'),
                               'two_odd_pointers': (-1, 'fq_kv_batch_decode_f16: pointer argument 0 of {kv_data, q_trans} is not 16-byte aligned')},
 'fq_kv_batch_decode_split': {'bad_layer': (-1, 'fq_kv_batch_decode_split: bad cache geometry'),
                              'negative_layer': (-1, 'fq_kv_batch_decode_split: bad cache geometry'),
                              'batch_0': (-1, 'fq_kv_batch_decode_split: bad cache geometry'),
                              'head_dim_96': (-2, 'fq_kv_batch_decode_split: head_dim=96 (64 or 128)'),
                              'page_size_0': (-1, 'fq_kv_batch_decode_split: bad cache geometry'),
                              'null_o': (-1, 'fq_kv_batch_decode_split: NULL pointer'),
                              'null_q': (-1, 'fq_kv_batch_decode_split: NULL pointer'),
                              'null_kv_data': (-1, 'fq_kv_batch_decode_split: NULL pointer'),
                              'null_kv_param': (-1, 'fq_kv_batch_decode_split: NULL pointer'),
                              'null_kv_param_fp16_cache': (-1,
                                                           'fq_kv_batch_decode_split: pointer argument 1 of {kv_data, q_trans, workspace} is not '
                                                           '16-byte aligned'),
                              'null_kv_indptr': (-1, 'fq_kv_batch_decode_split: NULL pointer'),
                              'null_kv_indices': (-1, 'fq_kv_batch_decode_split: NULL pointer'),
                              'null_last_page_offset': (-1, 'fq_kv_batch_decode_split: NULL pointer'),
                              'odd_kv_data': (-1,
                                              'fq_kv_batch_decode_split: pointer argument 0 of {kv_data, q_trans, workspace} is not 16-byte aligned'),
                              'odd_q_trans': (-1,
                                              'fq_kv_batch_decode_split: pointer argument 1 of {kv_data, q_trans, workspace} is not 16-byte aligned'),
                              'odd_workspace': (-1,
                                                'fq_kv_batch_decode_split: pointer argument 2 of {kv_data, q_trans, workspace} is not 16-byte '
                                                'aligned'),
                              'two_bad_layer_and_null': (-1, 'fq_kv_batch_decode_split: bad cache geometry'),
                              'two_head_dim_96_and_batch_0': (-1, 'fq_kv_batch_decode_split: bad cache geometry'),
                              'two_null_and_odd': (-1, 'fq_kv_batch_decode_split: NULL pointer'),
                              'two_odd_pointers': (-1,
                                                   'fq_kv_batch_decode_split: pointer argument 0 of {kv_data, q_trans, workspace} is not 16-byte '
                                                   'aligned'),
                              'workspace_one_short': (-1,
                                                      'fq_kv_batch_decode_split: workspace of 16655 bytes, fq_kv_decode_workspace_bytes says 16656'),
                              'workspace_bytes_0': (-1, 'fq_kv_batch_decode_split: workspace of 0 bytes, fq_kv_decode_workspace_bytes says 16656'),
                              'two_workspace_short_and_odd_workspace': (-1,
                                                                        'fq_kv_batch_decode_split: pointer argument 2 of {kv_data, q_trans, '
                                                                        'workspace} is not 16-byte aligned'),
                              'two_workspace_short_and_null': (-1, 'fq_kv_batch_decode_split: NULL pointer'),
                              'workspace_one_short_fp16_cache': (-1,
                                                                 'fq_kv_batch_decode_split: workspace of 16655 bytes, fq_kv_decode_workspace_bytes '
                                                                 'says 16656')},
 'fq_kv_batch_decode_gqa': {'bad_layer': (-1, 'fq_kv_batch_decode_gqa: bad cache geometry'),
                            'negative_layer': (-1, 'fq_kv_batch_decode_gqa: bad cache geometry'),
                            'batch_0': (-1, 'fq_kv_batch_decode_gqa: bad cache geometry'),
                            'head_dim_96': (-2, 'fq_kv_batch_decode_gqa: head_dim=96 (64 or 128)'),
                            'page_size_0': (-1, 'fq_kv_batch_decode_gqa: bad cache geometry'),
                            'null_o': (-1, 'fq_kv_batch_decode_gqa: NULL pointer'),
                            'null_q': (-1, 'fq_kv_batch_decode_gqa: NULL pointer'),
                            'null_kv_data': (-1, 'fq_kv_batch_decode_gqa: NULL pointer'),
                            'null_kv_param': (-1, 'fq_kv_batch_decode_gqa: NULL pointer'),
                            'null_kv_param_fp16_cache': (-1,
                                                         'fq_kv_batch_decode_gqa: pointer argument 1 of {kv_data, q_trans, workspace} is not 16-byte '
                                                         'aligned'),
                            'null_kv_indptr': (-1, 'fq_kv_batch_decode_gqa: NULL pointer'),
                            'null_kv_indices': (-1, 'fq_kv_batch_decode_gqa: NULL pointer'),
                            'null_last_page_offset': (-1, 'fq_kv_batch_decode_gqa: NULL pointer'),
                            'odd_kv_data': (-1, 'fq_kv_batch_decode_gqa: pointer argument 0 of {kv_data, q_trans, workspace} is not 16-byte aligned'),
                            'odd_q_trans': (-1, 'fq_kv_batch_decode_gqa: pointer argument 1 of {kv_data, q_trans, workspace} is not 16-byte aligned'),
                            'odd_workspace': (-1,
                                              'fq_kv_batch_decode_gqa: pointer argument 2 of {kv_data, q_trans, workspace} is not 16-byte aligned'),
                            'two_bad_layer_and_null': (-1, 'fq_kv_batch_decode_gqa: bad cache geometry'),
                            'two_head_dim_96_and_batch_0': (-1, 'fq_kv_batch_decode_gqa: bad cache geometry'),
                            'two_null_and_odd': (-1, 'fq_kv_batch_decode_gqa: NULL pointer'),
                            'two_odd_pointers': (-1,
                                                 'fq_kv_batch_decode_gqa: pointer argument 0 of {kv_data, q_trans, workspace} is not 16-byte '
                                                 'aligned'),
                            'q_group_0': (-1, 'fq_kv_batch_decode_gqa: q_group=0 out of [1, 64]'),
                            'q_group_65': (-1, 'fq_kv_batch_decode_gqa: q_group=65 out of [1, 64]'),
                            'two_q_group_65_and_null': (-1, 'fq_kv_batch_decode_gqa: q_group=65 out of [1, 64]'),
                            'two_q_group_0_and_bad_layer': (-1, 'fq_kv_batch_decode_gqa: bad cache geometry'),
                            'workspace_one_short': (-1,
                                                    'fq_kv_batch_decode_gqa: workspace of 16655 bytes, fq_kv_decode_workspace_bytes_gqa says 16656'),
                            'workspace_bytes_0': (-1, 'fq_kv_batch_decode_gqa: workspace of 0 bytes, fq_kv_decode_workspace_bytes_gqa says 16656'),
                            'two_workspace_short_and_odd_workspace': (-1,
                                                                      'fq_kv_batch_decode_gqa: pointer argument 2 of {kv_data, q_trans, workspace} '
                                                                      'is not 16-byte aligned'),
                            'two_workspace_short_and_null': (-1, 'fq_kv_batch_decode_gqa: NULL pointer'),
                            'workspace_one_short_fp16_cache': (-1,
                                                               'fq_kv_batch_decode_gqa: workspace of 16655 bytes, fq_kv_decode_workspace_bytes_gqa '
                                                               'says 16656'),
                            'workspace_one_short_merged': (-1,
                                                           'fq_kv_batch_decode_gqa: workspace of 1065471 bytes, fq_kv_decode_workspace_bytes_gqa '
                                                           'says 1065472')},
 'fq_kv_batch_decode_copies': {'bad_layer': (-1, 'fq_kv_batch_decode_copies: bad cache geometry'),
                               'negative_layer': (-1, 'fq_kv_batch_decode_copies: bad cache geometry'),
                               'batch_0': (-1, 'fq_kv_batch_decode_copies: bad cache geometry'),
                               'head_dim_96': (-2, 'fq_kv_batch_decode_copies: head_dim=96 (64 or 128)'),
                               'page_size_0': (-1, 'fq_kv_batch_decode_copies: bad cache geometry'),
                               'null_o': (-1, 'fq_kv_batch_decode_copies: NULL pointer'),
                               'null_q': (-1, 'fq_kv_batch_decode_copies: NULL pointer'),
                               'null_kv_data': (-1, 'fq_kv_batch_decode_copies: NULL pointer'),
                               'null_kv_param': (-1, 'fq_kv_batch_decode_copies: NULL pointer'),
                               'null_kv_param_fp16_cache': (-1,
                                                            'fq_kv_batch_decode_copies: pointer argument 1 of {kv_data, q_trans, workspace} is not '
                                                            '16-byte aligned'),
                               'null_kv_indptr': (-1, 'fq_kv_batch_decode_copies: NULL pointer'),
                               'null_kv_indices': (-1, 'fq_kv_batch_decode_copies: NULL pointer'),
                               'null_last_page_offset': (-1, 'fq_kv_batch_decode_copies: NULL pointer'),
                               'odd_kv_data': (-1,
                                               'fq_kv_batch_decode_copies: pointer argument 0 of {kv_data, q_trans, workspace} is not 16-byte '
                                               'aligned'),
                               'odd_q_trans': (-1,
                                               'fq_kv_batch_decode_copies: pointer argument 1 of {kv_data, q_trans, workspace} is not 16-byte '
                                               'aligned'),
                               'odd_workspace': (-1,
                                                 'fq_kv_batch_decode_copies: pointer argument 2 of {kv_data, q_trans, workspace} is not 16-byte '
                                                 'aligned'),
                               'two_bad_layer_and_null': (-1, 'fq_kv_batch_decode_copies: bad cache geometry'),
                               'two_head_dim_96_and_batch_0': (-1, 'fq_kv_batch_decode_copies: bad cache geometry'),
                               'two_null_and_odd': (-1, 'fq_kv_batch_decode_copies: NULL pointer'),
                               'two_odd_pointers': (-1,
                                                    'fq_kv_batch_decode_copies: pointer argument 0 of {kv_data, q_trans, workspace} is not 16-byte '
                                                    'aligned'),
                               'copies_9': (-1, 'fq_kv_batch_decode_copies: copies=9 must be 1..8 and divide num_heads=8'),
                               'copies_0': (-1, 'fq_kv_batch_decode_copies: copies=0 must be 1..8 and divide num_heads=8'),
                               'copies_not_dividing_heads': (-1, 'fq_kv_batch_decode_copies: copies=3 must be 1..8 and divide num_heads=8'),
                               'two_copies_9_and_null': (-1, 'fq_kv_batch_decode_copies: copies=9 must be 1..8 and divide num_heads=8'),
                               'workspace_one_short': (-1,
                                                       'fq_kv_batch_decode_copies: workspace of 16655 bytes, fq_kv_decode_workspace_bytes_gqa(batch, '
                                                       'num_heads / copies, copies, head_dim) says 16656'),
                               'workspace_bytes_0': (-1,
                                                     'fq_kv_batch_decode_copies: workspace of 0 bytes, fq_kv_decode_workspace_bytes_gqa(batch, '
                                                     'num_heads / copies, copies, head_dim) says 16656'),
                               'two_workspace_short_and_odd_workspace': (-1,
                                                                         'fq_kv_batch_decode_copies: pointer argument 2 of {kv_data, q_trans, '
                                                                         'workspace} is not 16-byte aligned'),
                               'two_workspace_short_and_null': (-1, 'fq_kv_batch_decode_copies: NULL pointer'),
                               'workspace_one_short_fp16_cache': (-1,
                                                                  'fq_kv_batch_decode_copies: workspace of 16655 bytes, '
                                                                  'fq_kv_decode_workspace_bytes_gqa(batch, num_heads / copies, copies, head_dim) '
                                                                  'says 16656'),
                               'workspace_one_short_copies_4': (-1,
                                                                'fq_kv_batch_decode_copies: workspace of 66591 bytes, '
                                                                'fq_kv_decode_workspace_bytes_gqa(batch, num_heads / copies, copies, head_dim) says '
                                                                '66592')},
 'fq_kv_decode_append_i4': {'bad_layer': (-1, 'fq_kv_decode_append_i4: bad cache geometry'),
                            'negative_layer': (-1, 'fq_kv_decode_append_i4: bad cache geometry'),
                            'batch_0': (-1, 'fq_kv_decode_append_i4: bad cache geometry'),
                            'head_dim_96': (-2, 'fq_kv_decode_append_i4: head_dim=96 (64 or 128)'),
                            'page_size_0': (-1, 'fq_kv_decode_append_i4: bad cache geometry'),
                            'null_o': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'null_q': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'null_k_new': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'null_v_new': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'null_kv_data': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'null_kv_param': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'null_kv_indptr': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'null_kv_indices': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'null_last_page_offset': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'odd_kv_data': (-1,
                                            'fq_kv_decode_append_i4: pointer argument 0 of {kv_data, q_trans, workspace, k_new, v_new, '
                                            'k_trans_image} is not 16-byte aligned'),
                            'odd_q_trans': (-1,
                                            'fq_kv_decode_append_i4: pointer argument 1 of {kv_data, q_trans, workspace, k_new, v_new, '
                                            'k_trans_image} is not 16-byte aligned'),
                            'odd_workspace': (-1,
                                              'fq_kv_decode_append_i4: pointer argument 2 of {kv_data, q_trans, workspace, k_new, v_new, '
                                              'k_trans_image} is not 16-byte aligned'),
                            'odd_k_new': (-1,
                                          'fq_kv_decode_append_i4: pointer argument 3 of {kv_data, q_trans, workspace, k_new, v_new, k_trans_image} '
                                          'is not 16-byte aligned'),
                            'odd_v_new': (-1,
                                          'fq_kv_decode_append_i4: pointer argument 4 of {kv_data, q_trans, workspace, k_new, v_new, k_trans_image} '
                                          'is not 16-byte aligned'),
                            'odd_k_trans_image': (-1,
                                                  'fq_kv_decode_append_i4: pointer argument 5 of {kv_data, q_trans, workspace, k_new, v_new, '
                                                  'k_trans_image} is not 16-byte aligned'),
                            'two_bad_layer_and_null': (-1, 'fq_kv_decode_append_i4: bad cache geometry'),
                            'two_head_dim_96_and_batch_0': (-1, 'fq_kv_decode_append_i4: bad cache geometry'),
                            'two_null_and_odd': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'two_odd_pointers': (-1,
                                                 'fq_kv_decode_append_i4: pointer argument 0 of {kv_data, q_trans, workspace, k_new, v_new, '
                                                 'k_trans_image} is not 16-byte aligned'),
                            'q_group_0': (-1, 'fq_kv_decode_append_i4: q_group=0 out of [1, 64]'),
                            'q_group_65': (-1, 'fq_kv_decode_append_i4: q_group=65 out of [1, 64]'),
                            'two_q_group_65_and_null': (-1, 'fq_kv_decode_append_i4: q_group=65 out of [1, 64]'),
                            'two_q_group_0_and_bad_layer': (-1, 'fq_kv_decode_append_i4: bad cache geometry'),
                            'page_size_8': (-2,
                                            'fq_kv_decode_append_i4: head_dim=128, page_size=8: needs head_dim 128 and page_size % 16 == 0 (use '
                                            'fq_kv_quant_append_i4 + the decode launch)'),
                            'head_dim_64': (-2,
                                            'fq_kv_decode_append_i4: head_dim=64, page_size=16: needs head_dim 128 and page_size % 16 == 0 (use '
                                            'fq_kv_quant_append_i4 + the decode launch)'),
                            'src_heads_0': (-1, 'fq_kv_decode_append_i4: num_kv_heads=8 must be src_heads=0 x a group of at most 8'),
                            'src_heads_not_dividing': (-1, 'fq_kv_decode_append_i4: num_kv_heads=8 must be src_heads=3 x a group of at most 8'),
                            'src_group_over_8': (-1, 'fq_kv_decode_append_i4: num_kv_heads=16 must be src_heads=1 x a group of at most 8'),
                            'two_page_size_8_and_q_group_65': (-1, 'fq_kv_decode_append_i4: q_group=65 out of [1, 64]'),
                            'two_page_size_8_and_src_heads_0': (-2,
                                                                'fq_kv_decode_append_i4: head_dim=128, page_size=8: needs head_dim 128 and page_size '
                                                                '% 16 == 0 (use fq_kv_quant_append_i4 + the decode launch)'),
                            'two_src_heads_0_and_null': (-1, 'fq_kv_decode_append_i4: num_kv_heads=8 must be src_heads=0 x a group of at most 8'),
                            'workspace_one_short': (-1,
                                                    'fq_kv_decode_append_i4: workspace of 16655 bytes, fq_kv_decode_workspace_bytes_gqa says 16656'),
                            'workspace_bytes_0': (-1, 'fq_kv_decode_append_i4: workspace of 0 bytes, fq_kv_decode_workspace_bytes_gqa says 16656'),
                            'two_workspace_short_and_odd_workspace': (-1,
                                                                      'fq_kv_decode_append_i4: pointer argument 2 of {kv_data, q_trans, workspace, '
                                                                      'k_new, v_new, k_trans_image} is not 16-byte aligned'),
                            'two_workspace_short_and_null': (-1, 'fq_kv_decode_append_i4: NULL pointer'),
                            'workspace_one_short_read_one_copy': (-1,
                                                                  'fq_kv_decode_append_i4: workspace of 66591 bytes, '
                                                                  'fq_kv_decode_workspace_bytes_gqa says 66592')},
 'fq_kv_decode_append_rope_i4': {'bad_layer': (-1, 'fq_kv_decode_append_rope_i4: bad cache geometry'),
                                 'negative_layer': (-1, 'fq_kv_decode_append_rope_i4: bad cache geometry'),
                                 'batch_0': (-1, 'fq_kv_decode_append_rope_i4: bad cache geometry'),
                                 'head_dim_96': (-2, 'fq_kv_decode_append_rope_i4: head_dim=96 (64 or 128)'),
                                 'page_size_0': (-1, 'fq_kv_decode_append_rope_i4: bad cache geometry'),
                                 'null_o': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'null_q': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'null_k_new': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'null_v_new': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'null_kv_data': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'null_kv_param': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'null_kv_indptr': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'null_kv_indices': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'null_last_page_offset': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'odd_kv_data': (-1,
                                                 'fq_kv_decode_append_rope_i4: pointer argument 0 of {kv_data, q_trans, workspace, k_new, v_new, '
                                                 'k_trans_image} is not 16-byte aligned'),
                                 'odd_q_trans': (-1,
                                                 'fq_kv_decode_append_rope_i4: pointer argument 1 of {kv_data, q_trans, workspace, k_new, v_new, '
                                                 'k_trans_image} is not 16-byte aligned'),
                                 'odd_workspace': (-1,
                                                   'fq_kv_decode_append_rope_i4: pointer argument 2 of {kv_data, q_trans, workspace, k_new, v_new, '
                                                   'k_trans_image} is not 16-byte aligned'),
                                 'odd_k_new': (-1,
                                               'fq_kv_decode_append_rope_i4: pointer argument 3 of {kv_data, q_trans, workspace, k_new, v_new, '
                                               'k_trans_image} is not 16-byte aligned'),
                                 'odd_v_new': (-1,
                                               'fq_kv_decode_append_rope_i4: pointer argument 4 of {kv_data, q_trans, workspace, k_new, v_new, '
                                               'k_trans_image} is not 16-byte aligned'),
                                 'odd_k_trans_image': (-1,
                                                       'fq_kv_decode_append_rope_i4: pointer argument 5 of {kv_data, q_trans, workspace, k_new, '
                                                       'v_new, k_trans_image} is not 16-byte aligned'),
                                 'odd_cos': (-1, 'fq_kv_decode_append_rope_i4: pointer argument 0 of {cos, sin} is not 16-byte aligned'),
                                 'odd_sin': (-1, 'fq_kv_decode_append_rope_i4: pointer argument 1 of {cos, sin} is not 16-byte aligned'),
                                 'two_bad_layer_and_null': (-1, 'fq_kv_decode_append_rope_i4: bad cache geometry'),
                                 'two_head_dim_96_and_batch_0': (-1, 'fq_kv_decode_append_rope_i4: bad cache geometry'),
                                 'two_null_and_odd': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'two_odd_pointers': (-1,
                                                      'fq_kv_decode_append_rope_i4: pointer argument 0 of {kv_data, q_trans, workspace, k_new, '
                                                      'v_new, k_trans_image} is not 16-byte aligned'),
                                 'q_group_0': (-1, 'fq_kv_decode_append_rope_i4: q_group=0 out of [1, 64]'),
                                 'q_group_65': (-1, 'fq_kv_decode_append_rope_i4: q_group=65 out of [1, 64]'),
                                 'two_q_group_65_and_null': (-1, 'fq_kv_decode_append_rope_i4: q_group=65 out of [1, 64]'),
                                 'two_q_group_0_and_bad_layer': (-1, 'fq_kv_decode_append_rope_i4: bad cache geometry'),
                                 'page_size_8': (-2,
                                                 'fq_kv_decode_append_rope_i4: head_dim=128, page_size=8: needs head_dim 128 and page_size % 16 == 0 '
                                                 '(use fq_kv_quant_append_i4 + the decode launch)'),
                                 'head_dim_64': (-2,
                                                 'fq_kv_decode_append_rope_i4: head_dim=64, page_size=16: needs head_dim 128 and page_size % 16 == 0 '
                                                 '(use fq_kv_quant_append_i4 + the decode launch)'),
                                 'src_heads_0': (-1, 'fq_kv_decode_append_rope_i4: num_kv_heads=8 must be src_heads=0 x a group of at most 8'),
                                 'src_heads_not_dividing': (-1,
                                                            'fq_kv_decode_append_rope_i4: num_kv_heads=8 must be src_heads=3 x a group of at most 8'),
                                 'src_group_over_8': (-1, 'fq_kv_decode_append_rope_i4: num_kv_heads=16 must be src_heads=1 x a group of at most 8'),
                                 'two_page_size_8_and_q_group_65': (-1, 'fq_kv_decode_append_rope_i4: q_group=65 out of [1, 64]'),
                                 'two_page_size_8_and_src_heads_0': (-2,
                                                                     'fq_kv_decode_append_rope_i4: head_dim=128, page_size=8: needs head_dim 128 and '
                                                                     'page_size % 16 == 0 (use fq_kv_quant_append_i4 + the decode launch)'),
                                 'two_src_heads_0_and_null': (-1,
                                                              'fq_kv_decode_append_rope_i4: num_kv_heads=8 must be src_heads=0 x a group of at most '
                                                              '8'),
                                 'cos_without_sin': (-1,
                                                     'fq_kv_decode_append_rope_i4: cos and sin go together (both, or neither for no rotary '
                                                     'embedding)'),
                                 'sin_without_cos': (-1,
                                                     'fq_kv_decode_append_rope_i4: cos and sin go together (both, or neither for no rotary '
                                                     'embedding)'),
                                 'two_cos_without_sin_and_odd_workspace': (-1,
                                                                           'fq_kv_decode_append_rope_i4: pointer argument 2 of {kv_data, q_trans, '
                                                                           'workspace, k_new, v_new, k_trans_image} is not 16-byte aligned'),
                                 'two_cos_without_sin_and_odd_cos': (-1,
                                                                     'fq_kv_decode_append_rope_i4: cos and sin go together (both, or neither for no '
                                                                     'rotary embedding)'),
                                 'two_cos_without_sin_and_null': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'two_odd_sin_and_short_workspace': (-1,
                                                                     'fq_kv_decode_append_rope_i4: pointer argument 1 of {cos, sin} is not 16-byte '
                                                                     'aligned'),
                                 'workspace_one_short': (-1,
                                                         'fq_kv_decode_append_rope_i4: workspace of 16655 bytes, fq_kv_decode_workspace_bytes_gqa '
                                                         'says 16656'),
                                 'workspace_bytes_0': (-1,
                                                       'fq_kv_decode_append_rope_i4: workspace of 0 bytes, fq_kv_decode_workspace_bytes_gqa says '
                                                       '16656'),
                                 'two_workspace_short_and_odd_workspace': (-1,
                                                                           'fq_kv_decode_append_rope_i4: pointer argument 2 of {kv_data, q_trans, '
                                                                           'workspace, k_new, v_new, k_trans_image} is not 16-byte aligned'),
                                 'two_workspace_short_and_null': (-1, 'fq_kv_decode_append_rope_i4: NULL pointer'),
                                 'workspace_one_short_read_one_copy': (-1,
                                                                       'fq_kv_decode_append_rope_i4: workspace of 66591 bytes, '
                                                                       'fq_kv_decode_workspace_bytes_gqa says 66592')},
 'fq_kv_decode_append_had_i4': {'bad_layer': (-1, 'fq_kv_decode_append_had_i4: bad cache geometry'),
                                'negative_layer': (-1, 'fq_kv_decode_append_had_i4: bad cache geometry'),
                                'batch_0': (-1, 'fq_kv_decode_append_had_i4: bad cache geometry'),
                                'head_dim_96': (-2, 'fq_kv_decode_append_had_i4: head_dim=96 (64 or 128)'),
                                'page_size_0': (-1, 'fq_kv_decode_append_had_i4: bad cache geometry'),
                                'null_o': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'null_q': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'null_k_new': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'null_v_new': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'null_kv_data': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'null_kv_param': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'null_kv_indptr': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'null_kv_indices': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'null_last_page_offset': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'odd_kv_data': (-1,
                                                'fq_kv_decode_append_had_i4: pointer argument 0 of {kv_data, q_trans, workspace, k_new, v_new, '
                                                'k_trans_image} is not 16-byte aligned'),
                                'odd_workspace': (-1,
                                                  'fq_kv_decode_append_had_i4: pointer argument 2 of {kv_data, q_trans, workspace, k_new, v_new, '
                                                  'k_trans_image} is not 16-byte aligned'),
                                'odd_k_new': (-1,
                                              'fq_kv_decode_append_had_i4: pointer argument 3 of {kv_data, q_trans, workspace, k_new, v_new, '
                                              'k_trans_image} is not 16-byte aligned'),
                                'odd_v_new': (-1,
                                              'fq_kv_decode_append_had_i4: pointer argument 4 of {kv_data, q_trans, workspace, k_new, v_new, '
                                              'k_trans_image} is not 16-byte aligned'),
                                'two_bad_layer_and_null': (-1, 'fq_kv_decode_append_had_i4: bad cache geometry'),
                                'two_head_dim_96_and_batch_0': (-1, 'fq_kv_decode_append_had_i4: bad cache geometry'),
                                'two_null_and_odd': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'two_odd_pointers': (-1,
                                                     'fq_kv_decode_append_had_i4: pointer argument 0 of {kv_data, q_trans, workspace, k_new, v_new, '
                                                     'k_trans_image} is not 16-byte aligned'),
                                'q_group_0': (-1, 'fq_kv_decode_append_had_i4: q_group=0 out of [1, 64]'),
                                'q_group_65': (-1, 'fq_kv_decode_append_had_i4: q_group=65 out of [1, 64]'),
                                'two_q_group_65_and_null': (-1, 'fq_kv_decode_append_had_i4: q_group=65 out of [1, 64]'),
                                'two_q_group_0_and_bad_layer': (-1, 'fq_kv_decode_append_had_i4: bad cache geometry'),
                                'page_size_8': (-2,
                                                'fq_kv_decode_append_had_i4: head_dim=128, page_size=8: needs head_dim 128 and page_size % 16 == 0 '
                                                '(use fq_kv_quant_append_i4 + the decode launch)'),
                                'head_dim_64': (-2,
                                                'fq_kv_decode_append_had_i4: head_dim=64, page_size=16: needs head_dim 128 and page_size % 16 == 0 '
                                                '(use fq_kv_quant_append_i4 + the decode launch)'),
                                'src_heads_0': (-1, 'fq_kv_decode_append_had_i4: num_kv_heads=8 must be src_heads=0 x a group of at most 8'),
                                'src_heads_not_dividing': (-1,
                                                           'fq_kv_decode_append_had_i4: num_kv_heads=8 must be src_heads=3 x a group of at most 8'),
                                'src_group_over_8': (-1, 'fq_kv_decode_append_had_i4: num_kv_heads=16 must be src_heads=1 x a group of at most 8'),
                                'two_page_size_8_and_q_group_65': (-1, 'fq_kv_decode_append_had_i4: q_group=65 out of [1, 64]'),
                                'two_page_size_8_and_src_heads_0': (-2,
                                                                    'fq_kv_decode_append_had_i4: head_dim=128, page_size=8: needs head_dim 128 and '
                                                                    'page_size % 16 == 0 (use fq_kv_quant_append_i4 + the decode launch)'),
                                'two_src_heads_0_and_null': (-1,
                                                             'fq_kv_decode_append_had_i4: num_kv_heads=8 must be src_heads=0 x a group of at most 8'),
                                'workspace_one_short': (-1,
                                                        'fq_kv_decode_append_had_i4: workspace of 16655 bytes, fq_kv_decode_workspace_bytes_gqa says '
                                                        '16656'),
                                'workspace_bytes_0': (-1,
                                                      'fq_kv_decode_append_had_i4: workspace of 0 bytes, fq_kv_decode_workspace_bytes_gqa says '
                                                      '16656'),
                                'two_workspace_short_and_odd_workspace': (-1,
                                                                          'fq_kv_decode_append_had_i4: pointer argument 2 of {kv_data, q_trans, '
                                                                          'workspace, k_new, v_new, k_trans_image} is not 16-byte aligned'),
                                'two_workspace_short_and_null': (-1, 'fq_kv_decode_append_had_i4: NULL pointer'),
                                'workspace_one_short_read_one_copy': (-1,
                                                                      'fq_kv_decode_append_had_i4: workspace of 66591 bytes, '
                                                                      'fq_kv_decode_workspace_bytes_gqa says 66592')},
 'fq_kv_batch_extend': {'bad_layer': (-1, 'fq_kv_batch_extend: bad cache geometry'),
                        'negative_layer': (-1, 'fq_kv_batch_extend: bad cache geometry'),
                        'batch_0': (-1, 'fq_kv_batch_extend: bad cache geometry'),
                        'head_dim_96': (-2, 'fq_kv_batch_extend: head_dim=96 (64 or 128)'),
                        'page_size_0': (-1, 'fq_kv_batch_extend: bad cache geometry'),
                        'null_o': (-1, 'fq_kv_batch_extend: NULL pointer'),
                        'null_q': (-1, 'fq_kv_batch_extend: NULL pointer'),
                        'null_kv_data': (-1, 'fq_kv_batch_extend: NULL pointer'),
                        'null_kv_param': (-1, 'fq_kv_batch_extend: NULL pointer'),
                        'null_kv_param_fp16_cache': (-1,
                                                     'fq_kv_batch_extend: pointer argument 1 of {kv_data, q_trans, workspace} is not 16-byte '
                                                     'aligned'),
                        'null_kv_indptr': (-1, 'fq_kv_batch_extend: NULL pointer'),
                        'null_kv_indices': (-1, 'fq_kv_batch_extend: NULL pointer'),
                        'null_last_page_offset': (-1, 'fq_kv_batch_extend: NULL pointer'),
                        'odd_kv_data': (-1, 'fq_kv_batch_extend: pointer argument 0 of {kv_data, q_trans, workspace} is not 16-byte aligned'),
                        'odd_q_trans': (-1, 'fq_kv_batch_extend: pointer argument 1 of {kv_data, q_trans, workspace} is not 16-byte aligned'),
                        'odd_workspace': (-1, 'fq_kv_batch_extend: pointer argument 2 of {kv_data, q_trans, workspace} is not 16-byte aligned'),
                        'two_bad_layer_and_null': (-1, 'fq_kv_batch_extend: bad cache geometry'),
                        'two_head_dim_96_and_batch_0': (-1, 'fq_kv_batch_extend: bad cache geometry'),
                        'two_null_and_odd': (-1, 'fq_kv_batch_extend: NULL pointer'),
                        'two_odd_pointers': (-1, 'fq_kv_batch_extend: pointer argument 0 of {kv_data, q_trans, workspace} is not 16-byte aligned'),
                        'q_group_0': (-1,
                                      'fq_kv_batch_extend: q_group=0 (1..64) must be a multiple of copies=1 (1..8), which must divide '
                                      'num_cache_heads=8'),
                        'q_group_65': (-1,
                                       'fq_kv_batch_extend: q_group=65 (1..64) must be a multiple of copies=1 (1..8), which must divide '
                                       'num_cache_heads=8'),
                        'two_q_group_65_and_null': (-1,
                                                    'fq_kv_batch_extend: q_group=65 (1..64) must be a multiple of copies=1 (1..8), which must divide '
                                                    'num_cache_heads=8'),
                        'two_q_group_0_and_bad_layer': (-1, 'fq_kv_batch_extend: bad cache geometry'),
                        'copies_9': (-1,
                                     'fq_kv_batch_extend: q_group=9 (1..64) must be a multiple of copies=9 (1..8), which must divide '
                                     'num_cache_heads=8'),
                        'copies_0': (-1,
                                     'fq_kv_batch_extend: q_group=4 (1..64) must be a multiple of copies=0 (1..8), which must divide '
                                     'num_cache_heads=8'),
                        'copies_not_dividing_heads': (-1,
                                                      'fq_kv_batch_extend: q_group=3 (1..64) must be a multiple of copies=3 (1..8), which must '
                                                      'divide num_cache_heads=8'),
                        'two_copies_9_and_null': (-1,
                                                  'fq_kv_batch_extend: q_group=4 (1..64) must be a multiple of copies=9 (1..8), which must divide '
                                                  'num_cache_heads=8'),
                        'q_group_not_multiple_of_copies': (-1,
                                                           'fq_kv_batch_extend: q_group=4 (1..64) must be a multiple of copies=8 (1..8), which must '
                                                           'divide num_cache_heads=8'),
                        'q_len_0': (-1, 'fq_kv_batch_extend: q_len=0 must be >= 1'),
                        'two_q_len_0_and_bad_layer': (-1, 'fq_kv_batch_extend: q_len=0 must be >= 1'),
                        'head_dim_64': (-2, 'fq_kv_batch_extend: head_dim=64 (128 only)'),
                        'two_head_dim_64_and_copies_9': (-1,
                                                         'fq_kv_batch_extend: q_group=4 (1..64) must be a multiple of copies=9 (1..8), which must '
                                                         'divide num_cache_heads=8'),
                        'two_head_dim_64_and_null': (-2, 'fq_kv_batch_extend: head_dim=64 (128 only)'),
                        'workspace_one_short': (-1, 'fq_kv_batch_extend: workspace of 2130431 bytes, fq_kv_extend_workspace_bytes says 2130432'),
                        'workspace_bytes_0': (-1, 'fq_kv_batch_extend: workspace of 0 bytes, fq_kv_extend_workspace_bytes says 2130432'),
                        'two_workspace_short_and_odd_workspace': (-1,
                                                                  'fq_kv_batch_extend: pointer argument 2 of {kv_data, q_trans, workspace} is not '
                                                                  '16-byte aligned'),
                        'two_workspace_short_and_null': (-1, 'fq_kv_batch_extend: NULL pointer'),
                        'workspace_one_short_fp16_cache': (-1,
                                                           'fq_kv_batch_extend: workspace of 2130431 bytes, fq_kv_extend_workspace_bytes says '
                                                           '2130432')},
 'fq_kv_chunk_extend': {'bad_layer': (-1, 'fq_kv_chunk_extend: bad cache geometry'),
                        'negative_layer': (-1, 'fq_kv_chunk_extend: bad cache geometry'),
                        'batch_0': (-1, 'fq_kv_chunk_extend: bad cache geometry'),
                        'head_dim_96': (-2, 'fq_kv_chunk_extend: head_dim=96 (64 or 128)'),
                        'page_size_0': (-1, 'fq_kv_chunk_extend: bad cache geometry'),
                        'null_o': (-1, 'fq_kv_chunk_extend: NULL pointer'),
                        'null_q': (-1, 'fq_kv_chunk_extend: NULL pointer'),
                        'null_kv_data': (-1, 'fq_kv_chunk_extend: NULL pointer'),
                        'null_kv_param': (-1, 'fq_kv_chunk_extend: NULL pointer'),
                        'null_kv_param_fp16_cache': (-1, 'fq_kv_chunk_extend: pointer argument 3 of {o, q, kv_data, q_trans} is not 16-byte aligned'),
                        'null_kv_indptr': (-1, 'fq_kv_chunk_extend: NULL pointer'),
                        'null_kv_indices': (-1, 'fq_kv_chunk_extend: NULL pointer'),
                        'null_last_page_offset': (-1, 'fq_kv_chunk_extend: NULL pointer'),
                        'odd_o': (-1, 'fq_kv_chunk_extend: pointer argument 0 of {o, q, kv_data, q_trans} is not 16-byte aligned'),
                        'odd_q': (-1, 'fq_kv_chunk_extend: pointer argument 1 of {o, q, kv_data, q_trans} is not 16-byte aligned'),
                        'odd_kv_data': (-1, 'fq_kv_chunk_extend: pointer argument 2 of {o, q, kv_data, q_trans} is not 16-byte aligned'),
                        'odd_q_trans': (-1, 'fq_kv_chunk_extend: pointer argument 3 of {o, q, kv_data, q_trans} is not 16-byte aligned'),
                        'two_bad_layer_and_null': (-1, 'fq_kv_chunk_extend: bad cache geometry'),
                        'two_head_dim_96_and_batch_0': (-1, 'fq_kv_chunk_extend: bad cache geometry'),
                        'two_null_and_odd': (-1, 'fq_kv_chunk_extend: NULL pointer'),
                        'two_odd_pointers': (-1, 'fq_kv_chunk_extend: pointer argument 0 of {o, q, kv_data, q_trans} is not 16-byte aligned'),
                        'q_group_0': (-1,
                                      'fq_kv_chunk_extend: q_group=0 (1..64) must be a multiple of copies=1 (1..8), which must divide '
                                      'num_cache_heads=8'),
                        'q_group_65': (-1,
                                       'fq_kv_chunk_extend: q_group=65 (1..64) must be a multiple of copies=1 (1..8), which must divide '
                                       'num_cache_heads=8'),
                        'two_q_group_65_and_null': (-1,
                                                    'fq_kv_chunk_extend: q_group=65 (1..64) must be a multiple of copies=1 (1..8), which must divide '
                                                    'num_cache_heads=8'),
                        'two_q_group_0_and_bad_layer': (-1, 'fq_kv_chunk_extend: bad cache geometry'),
                        'copies_9': (-1,
                                     'fq_kv_chunk_extend: q_group=9 (1..64) must be a multiple of copies=9 (1..8), which must divide '
                                     'num_cache_heads=8'),
                        'copies_0': (-1,
                                     'fq_kv_chunk_extend: q_group=4 (1..64) must be a multiple of copies=0 (1..8), which must divide '
                                     'num_cache_heads=8'),
                        'copies_not_dividing_heads': (-1,
                                                      'fq_kv_chunk_extend: q_group=3 (1..64) must be a multiple of copies=3 (1..8), which must '
                                                      'divide num_cache_heads=8'),
                        'two_copies_9_and_null': (-1,
                                                  'fq_kv_chunk_extend: q_group=4 (1..64) must be a multiple of copies=9 (1..8), which must divide '
                                                  'num_cache_heads=8'),
                        'q_group_not_multiple_of_copies': (-1,
                                                           'fq_kv_chunk_extend: q_group=4 (1..64) must be a multiple of copies=8 (1..8), which must '
                                                           'divide num_cache_heads=8'),
                        'q_len_0': (-1, 'fq_kv_chunk_extend: q_len=0 must be >= 1'),
                        'two_q_len_0_and_bad_layer': (-1, 'fq_kv_chunk_extend: q_len=0 must be >= 1'),
                        'head_dim_64': (-2, 'fq_kv_chunk_extend: head_dim=64 (128 only)'),
                        'two_head_dim_64_and_copies_9': (-1,
                                                         'fq_kv_chunk_extend: q_group=4 (1..64) must be a multiple of copies=9 (1..8), which must '
                                                         'divide num_cache_heads=8'),
                        'two_head_dim_64_and_null': (-2, 'fq_kv_chunk_extend: head_dim=64 (128 only)'),
                        'q_group_3': (-2, 'fq_kv_chunk_extend: q_group=3 (1, 2, 4 or 8; fq_kv_batch_extend takes any group)'),
                        'two_q_group_3_and_null': (-2, 'fq_kv_chunk_extend: q_group=3 (1, 2, 4 or 8; fq_kv_batch_extend takes any group)'),
                        'two_q_group_3_and_head_dim_64': (-2, 'fq_kv_chunk_extend: head_dim=64 (128 only)'),
                        'too_many_rows': (-1, 'fq_kv_chunk_extend: batch_size=2 x 8 row sets x q_len=2147483647 is more than one launch takes'),
                        'two_too_many_rows_and_odd_q': (-1,
                                                        'fq_kv_chunk_extend: pointer argument 1 of {o, q, kv_data, q_trans} is not 16-byte aligned')},
 'fq_prefill_attention_f16': {'head_dim_64': (-2, 'fq_prefill_attention_f16: head_dim=64 (128 only)'),
                              'head_dim_96': (-1, 'fq_prefill_attention_f16: head_dim=96 (128 only)'),
                              'batch_0': (-1,
                                          'fq_prefill_attention_f16: batch_size=0, seq=130, q_heads=8, kv_heads=2: all >= 1, q_heads a multiple of '
                                          'kv_heads'),
                              'seq_0': (-1,
                                        'fq_prefill_attention_f16: batch_size=2, seq=0, q_heads=8, kv_heads=2: all >= 1, q_heads a multiple of '
                                        'kv_heads'),
                              'heads_not_multiple': (-1,
                                                     'fq_prefill_attention_f16: batch_size=2, seq=130, q_heads=7, kv_heads=2: all >= 1, q_heads a '
                                                     'multiple of kv_heads'),
                              'seq_start_alone': (-1, 'fq_prefill_attention_f16: seq_start and seq_len go together (both or neither)'),
                              'seq_len_alone': (-1, 'fq_prefill_attention_f16: seq_start and seq_len go together (both or neither)'),
                              'null_o': (-1, 'fq_prefill_attention_f16: NULL pointer'),
                              'null_q': (-1, 'fq_prefill_attention_f16: NULL pointer'),
                              'null_k': (-1, 'fq_prefill_attention_f16: NULL pointer'),
                              'null_v': (-1, 'fq_prefill_attention_f16: NULL pointer'),
                              'odd_o': (-1,
                                        'fq_prefill_attention_f16: pointer argument 0 of {o, q, q_trans, k, v, seq_start, seq_len} is not 16-byte '
                                        'aligned'),
                              'odd_q': (-1,
                                        'fq_prefill_attention_f16: pointer argument 1 of {o, q, q_trans, k, v, seq_start, seq_len} is not 16-byte '
                                        'aligned'),
                              'odd_q_trans': (-1,
                                              'fq_prefill_attention_f16: pointer argument 2 of {o, q, q_trans, k, v, seq_start, seq_len} is not '
                                              '16-byte aligned'),
                              'odd_k': (-1,
                                        'fq_prefill_attention_f16: pointer argument 3 of {o, q, q_trans, k, v, seq_start, seq_len} is not 16-byte '
                                        'aligned'),
                              'odd_v': (-1,
                                        'fq_prefill_attention_f16: pointer argument 4 of {o, q, q_trans, k, v, seq_start, seq_len} is not 16-byte '
                                        'aligned'),
                              'odd_seq_start': (-1,
                                                'fq_prefill_attention_f16: pointer argument 5 of {o, q, q_trans, k, v, seq_start, seq_len} is not '
                                                '16-byte aligned'),
                              'odd_seq_len': (-1,
                                              'fq_prefill_attention_f16: pointer argument 6 of {o, q, q_trans, k, v, seq_start, seq_len} is not '
                                              '16-byte aligned'),
                              'two_odd_v_and_head_dim_64': (-1,
                                                            'fq_prefill_attention_f16: pointer argument 4 of {o, q, q_trans, k, v, seq_start, '
                                                            'seq_len} is not 16-byte aligned'),
                              'two_head_dim_64_and_batch_0': (-2, 'fq_prefill_attention_f16: head_dim=64 (128 only)'),
                              'two_seq_start_alone_and_null_o': (-1,
                                                                 'fq_prefill_attention_f16: seq_start and seq_len go together (both or neither)')}}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_rejected_calls_keep_code_and_message(entry):
    from flatquant_amd._lib import lib
    table = cases(entry)
    assert [cid for cid, _ in table] == list(EXPECTED[entry]), "the case table and the recorded table list different cases"
    for cid, changes in table:
        assert call(lib, entry, changes) == EXPECTED[entry][cid], (entry, cid)


def test_every_required_fault_is_in_the_table():
    """the faults the table must hold, by entry point (a case removed from cases() would otherwise go unnoticed with its record)"""
    for entry in ENTRIES:
        ids = {cid for cid, _ in cases(entry)}
        assert any(c.startswith("two_") for c in ids), entry
        if entry == "fq_prefill_attention_f16":
            continue
        names = [n for n, _ in ENTRIES[entry]]
        assert {"bad_layer", "batch_0", "head_dim_96", "null_kv_param", "odd_kv_data"} <= ids, entry
        assert {f"null_{n}" for n in names if n in _POINTERS and n not in _OPTIONAL} <= ids, entry
        if "fp16_cache" in names:
            assert "null_kv_param_fp16_cache" in ids, entry
        if "q_group" in names:
            assert {"q_group_0", "q_group_65"} <= ids, entry
        if "copies" in names:
            assert {"copies_9", "copies_not_dividing_heads"} <= ids, entry
        if "workspace_bytes" in names:
            assert "workspace_one_short" in ids, entry
    assert "q_group_3" in {c for c, _ in cases("fq_kv_chunk_extend")}
    assert "q_group_not_multiple_of_copies" in {c for c, _ in cases("fq_kv_batch_extend")}
    assert "cos_without_sin" in {c for c, _ in cases("fq_kv_decode_append_rope_i4")}
    assert "page_size_8" in {c for c, _ in cases("fq_kv_decode_append_i4")}
    assert "tokens_not_multiple_of_batch" in {c for c, _ in cases("fq_kv_quant_append_i4")}


def test_workspace_sizes():
    from flatquant_amd._lib import lib
    assert workspace_sizes(lib) == WORKSPACE_SIZES


if __name__ == "__main__":   # print both tables for the loaded library
    import os
    import pprint
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from flatquant_amd._lib import lib as _lib
    _expected = {}
    for _entry in ENTRIES:
        _expected[_entry] = {}
        for _cid, _changes in cases(_entry):
            _code, _msg = call(_lib, _entry, _changes)
            assert _code in (-1, -2), (_entry, _cid, _code, _msg)   # FQ_EINVAL / FQ_EUNSUPPORTED: a case that passes validation has no place here
            _expected[_entry][_cid] = (_code, _msg)
    print("WORKSPACE_SIZES = " + pprint.pformat(workspace_sizes(_lib), width=150, compact=True))
    print("\nEXPECTED = " + pprint.pformat(_expected, width=150, sort_dicts=False))
