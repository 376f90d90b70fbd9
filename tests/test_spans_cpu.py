"""Per-token byte spans (include/tekken_hip.h tk_token_spans_device), the parts that need no GPU: the numpy restatement of the
definition that tests/test_gpu_spans.py checks the kernel against, the Rust shim's declarations, and the host-only tokenizer."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tk_token_spans_device", "tk_encode_batch_device_spans", "tk_encode_batch_spans", "tk_free_spans",
               "tk_tokenizer_encode_with_spans"]


def expected_spans(ids, id_offs, tok_len, num_special):
    """The definition, restated: per document, an exclusive prefix sum of the ids' byte lengths (tok_len by rank, from the Python
    token list; a special id: 0).  -> uint32[n_ids, 2] of (start, end), relative to the start of the id's document."""
    ids = np.asarray(ids, np.int64)
    id_offs = np.asarray(id_offs, np.int64)
    lens = np.zeros(len(ids), np.int64)
    body = ids >= num_special
    lens[body] = np.asarray(tok_len, np.int64)[ids[body] - num_special]
    incl = np.concatenate([[0], np.cumsum(lens)])
    doc_of = np.repeat(np.arange(len(id_offs) - 1), np.diff(id_offs))
    start = incl[:-1] - incl[id_offs[:-1]][doc_of]
    return np.stack([start, start + lens], axis=1).astype(np.uint32).reshape(len(ids), 2)


def test_restatement_hand_made():
    # ranks: 0 'a' (1 byte), 1 'hello' (5), 2 ' world' (6), 3 '\xf0\x9f' (2); three specials (0 = <unk>, 1 = BOS, 2 = EOS)
    tok_len = [1, 5, 6, 2]
    ns = 3
    a, hello, world, half = 3, 4, 5, 6
    ids = [1, hello, world, 2,            # doc 0: BOS hello world EOS
           a, a, half, half,              # doc 1: two bytes and two halves of an emoji
           # doc 2: empty
           1, 2,                          # doc 3: BOS EOS of an empty text
           hello, 0, a]                   # doc 4: a special in the middle
    offs = [0, 4, 8, 8, 10, 13]
    got = expected_spans(ids, offs, tok_len, ns)
    assert got.tolist() == [[0, 0], [0, 5], [5, 11], [11, 11],
                            [0, 1], [1, 2], [2, 4], [4, 6],
                            [0, 0], [0, 0],
                            [0, 5], [5, 5], [5, 6]]
    assert expected_spans([], [0, 0, 0], tok_len, ns).shape == (0, 2)


def test_restatement_tiles_random_documents():
    rng = np.random.default_rng(5)
    tok_len = rng.integers(1, 20, 300)
    ns = 10
    counts = rng.integers(0, 40, 50)
    offs = np.concatenate([[0], np.cumsum(counts)])
    ids = rng.integers(0, ns + len(tok_len), int(offs[-1]))
    sp = expected_spans(ids, offs, tok_len, ns).astype(np.int64)
    for d in range(len(counts)):
        s = sp[offs[d]:offs[d + 1]]
        want = sum(int(tok_len[i - ns]) for i in ids[offs[d]:offs[d + 1]] if i >= ns)
        if len(s):
            assert s[0, 0] == 0 and s[-1, 1] == want and np.all(s[1:, 0] == s[:-1, 1])


def test_new_symbols_declared_in_header_and_shim():
    hdr = open(os.path.join(ROOT, "include", "tekken_hip.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bfn\s+%s\s*\(" % name, ffi), name
    assert re.search(r"#define TK_SPANS_CHECK_COVER 4\b", hdr) and re.search(r"#define TK_SPANS_CHECK_BYTES 8\b", hdr)


def test_host_only_tokenizer_has_no_offsets(tk, small_vocab):
    from test_host_tokenizer import model
    t = tk.Tekkenizer.from_json(json.dumps(model(small_vocab["tokens"])), device=-1)
    with pytest.raises(tk.TokenizerError) as e:
        t.encode_with_offsets("hello world", True, True)
    assert e.value.code == tk.TK_ERR_NO_DEVICE
    with pytest.raises(tk.TokenizerError) as e:
        t.encode_batch_with_offsets(["hello world"])
    assert e.value.code == tk.TK_ERR_NO_DEVICE
    t.close()
