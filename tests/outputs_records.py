"""The designed records of the outputs' lab tests (tests/test_gpu_outputs.py) and of the probe that times the combined pass
(profiles/probe/outputs_pass.py; the LEDGER's "Combined outputs" figures are taken over lab_records(default_rng(4096), 4096, K)).
Plain module, no GPU: the text sink's designed records (tests/test_gpu_text_sink.py designed_records) put on 1000 channels, with
REAL equal keys, every text length of 58 .. 65, and texts of every escape class of json_model."""
import numpy as np

NCH_LAB = 1000
CHNS_LAB = (0, 8, 98, 998)
T0_LAB = (10 ** 9, 79)
TEXT_LENS_WANTED = (0, 1, 58, 59, 60, 61, 62, 63, 64, 65, 241, 242)
JSON_CLASSES = np.concatenate([np.array([1, 2, 4, 5, 6, 7, 0x0B, 0x0E, 0x1B, 0x1F], dtype=np.uint8), np.frombuffer(b'"\\\b\f\n\r\t', dtype=np.uint8),
                               np.frombuffer(b"ABCXYZ019 ,./-abc~\x7f\x80\xff", dtype=np.uint8), np.zeros(2, dtype=np.uint8)])


def lab_records(rng, n, K):
    """n acg_msg records as rows of bytes.  Record i sits on channel CHNS_LAB[i % 4]; records with i % 5 in (3, 4) take the
    end_bit of record i - 4, which is on the same channel: runs of two and three records under ONE (chn, end_bit) key at distinct
    input positions (designed_records' own repeats land on another channel here and make none).  txt_len 61 and 62 are added to
    designed_records' 0, 1, 58, 59, 60, 63, 64, 65, 241, 242; every ninth text is drawn from all of json_model's escape classes
    (\\u00xx, the two-byte escapes, plain bytes, NUL).  Records marked dropped (reserved2) and labels that decode are
    designed_records'."""
    from test_gpu_text_sink import designed_records
    recs = designed_records(rng, n, K)
    M = K.Msg
    word = lambda v, dt: np.frombuffer(np.array(v, dtype=dt).tobytes(), dtype=np.uint8)
    for i in range(n):
        recs[i, M.chn.offset:M.chn.offset + 4] = word(CHNS_LAB[i % 4], np.int32)
        if i % 5 in (3, 4) and i >= 4:
            recs[i, M.end_bit.offset:M.end_bit.offset + 8] = recs[i - 4, M.end_bit.offset:M.end_bit.offset + 8]
        if i % 9 == 5:
            recs[i, M.txt.offset:M.txt.offset + 242] = JSON_CLASSES[rng.integers(0, len(JSON_CLASSES), 242)]
        if i % 17 in (1, 2) and i % 7 != 4 and i % 61 != 60:         # (not a record whose label decodes, not a clamped length)
            recs[i, M.txt_len.offset:M.txt_len.offset + 4] = word(60 + i % 17, np.int32)
    return recs


def key_of(m):
    return (m.chn << 44) | m.end_bit


def equal_key_pairs(kept):
    """kept: the kept records in handed-out order.  (pairs inside a 256-rank workgroup, pairs across two): neighbours in rank
    under one key"""
    inside = across = 0
    for r in range(1, len(kept)):
        if key_of(kept[r]) == key_of(kept[r - 1]):
            if r % 256 == 0:
                across += 1
            else:
                inside += 1
    return inside, across
