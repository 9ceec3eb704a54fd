"""mspa.sampling.sample_dataframe against the reference's (same global NumPy seed, same rows out).

The reference's rows are frozen in tests/golden/sampling.npz (oracle/gen_golden.py); where the reference is mounted it is
also run live, and its rows must still be the frozen ones."""
import numpy as np
import pandas as pd
import pytest

from golden_util import GOLDEN_DIR
from mspa.sampling import sample_dataframe
from oracle import ref_harness as RH
from oracle.gen_golden import SAMPLING_CASES, SAMPLING_NP_SEED, sampling_frame


@pytest.mark.parametrize("case", range(len(SAMPLING_CASES)),
                         ids=["-".join(str(v) for v in c) for c in SAMPLING_CASES])
def test_sample_dataframe(case, capsys):
    seed, n, total, zeros, lo, hi, step = SAMPLING_CASES[case]
    df = sampling_frame(seed, n)
    gold = np.load(f"{GOLDEN_DIR}/sampling.npz")
    assert gold["cases"][case].tolist() == list(SAMPLING_CASES[case])
    want = df.iloc[gold[f"rows_{case}"]].reset_index(drop=True)
    if RH.reference_available():
        ref = RH.import_reference()
        np.random.seed(SAMPLING_NP_SEED)
        live = ref.CME.sample_dataframe(df, total, zeros, lo, hi, step)
        pd.testing.assert_frame_equal(live.reset_index(drop=True), want)
    np.random.seed(SAMPLING_NP_SEED)
    got = sample_dataframe(df, total, zeros, lo, hi, step)
    pd.testing.assert_frame_equal(got.reset_index(drop=True), want)
