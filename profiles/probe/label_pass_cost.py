"""What the batch sink's label pass (label.hip: filter, label decoding, compaction) costs beside the demodulator: a collect loop
(lag 1 after every call) with a filter and OOOI at the widths given on the command line, label traffic from the label fixture on
every channel.  Run under

    rocprofv3 --kernel-trace --stats -d <dir> -o labels -- python profiles/probe/label_pass_cost.py 1024 16384

and read msg_keep_count_kernel + msg_compact_kernel per collect against the demodulator's launches of the same calls
(profiles/LEDGER.md).  Prints per width: calls, collects, messages handed out, kept."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from acarsdec_amd import decoder as D  # noqa: E402

CHUNK, NCALL = 8192, 8


def run(nch):
    pcm = np.load(os.path.join(ROOT, "tests", "golden", "labels_pcm16.npz"))["pcm"].astype(np.float32) / 32768.0
    rng = np.random.default_rng(nch)
    n = CHUNK * NCALL
    base = np.stack([np.roll(pcm, -int(rng.integers(0, pcm.size)))[:n] for _ in range(64)])
    x = torch.from_numpy(base).cuda().repeat(nch // 64, 1).contiguous()
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=CHUNK // 1024, repair=True, bitlog=False, max_lag=1)
    dec.set_msg_filter(skip_empty=True, labels="Q1:QA:QB:QC:QD:44:26:RB:8E:H1:10:2Z")
    got = 0
    for k in range(NCALL + 1):
        if k < NCALL:
            p = x.data_ptr() + 4 * k * CHUNK
            dec._chk(dec.L.acg_process_dm_dev(dec.ctx, p, n, CHUNK, None))
        got += len(dec.collect_msgs(lag=1 if k < NCALL else 0, oooi=True))
    dec.close()
    print("nch %d: %d calls, %d collects, %d messages kept" % (nch, NCALL, NCALL + 1, got), flush=True)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["1024"]:
        run(int(w))
