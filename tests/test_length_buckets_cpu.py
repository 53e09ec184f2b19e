"""Bucket lists of the length-masked training step (train.check_buckets / pick_bucket) and the LENGTH_BUCKETS config key: no GPU."""
import pytest

from spoofsv_amd import train


def test_text2mel_buckets_are_validated_and_sorted():
    assert train.check_buckets("text2mel", [[186, 325], (64, 96), [128, 192]], 186, 325) == [(64, 96), (128, 192), (186, 325)]


def test_ssrn_buckets_take_plain_frame_counts():
    assert train.check_buckets("ssrn", [325, 96, [192]], 186, 325) == [(96,), (192,), (325,)]


@pytest.mark.parametrize("kind,bad", [
    ("text2mel", [[187, 325]]),          # above MAX_TEXT_LEN
    ("text2mel", [[64, 326]]),           # above MAX_FRAME_NUM
    ("ssrn", [326]),
    ("text2mel", [[64]]),                # not a pair
    ("text2mel", [64, 96]),
    ("text2mel", [[64, 96, 1]]),
    ("ssrn", [[64, 96]]),
    ("text2mel", [[0, 96]]),
    ("ssrn", [-3]),
    ("ssrn", [96.5]),
    ("ssrn", [True]),
    ("ssrn", ["96"]),
    ("ssrn", []),
    ("ssrn", [96, 96]),
    ("ssrn", 96),
    ("ssrn", "96"),
])
def test_malformed_or_oversized_buckets_are_refused(kind, bad):
    with pytest.raises(ValueError):
        train.check_buckets(kind, bad, 186, 325)


def test_unknown_kind_is_refused():
    with pytest.raises(ValueError):
        train.check_buckets("critic", [96])


def test_smallest_bucket_that_holds_the_batch_is_picked():
    b = train.check_buckets("text2mel", [[186, 325], [64, 96], [128, 192], [64, 325]], 186, 325)
    assert train.pick_bucket(b, (64, 96)) == (64, 96)
    assert train.pick_bucket(b, (65, 96)) == (128, 192)
    assert train.pick_bucket(b, (20, 200)) == (64, 325)
    assert train.pick_bucket(b, (101, 157)) == (128, 192)
    assert train.pick_bucket(b, (186, 325)) == (186, 325)
    assert train.pick_bucket(b, (187, 10)) is None         # larger than every bucket: the eager fallback
    s = train.check_buckets("ssrn", [192, 96], 186, 325)
    assert train.pick_bucket(s, (96,)) == (96,) and train.pick_bucket(s, (97,)) == (192,) and train.pick_bucket(s, (193,)) is None


@pytest.mark.parametrize("step,buckets", [("train_text2mel", [[500, 96]]), ("train_text2mel", [96]), ("train_ssrn", [[64, 96]]),
                                          ("train_ssrn", [1000])])
def test_ordinary_train_refuses_bad_length_buckets_before_any_work(step, buckets):
    import json
    import os
    from spoofsv_amd import harness
    cfg = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config.json")))
    cfg["LENGTH_BUCKETS"] = buckets
    with pytest.raises(ValueError):
        harness.ordinary_train(step, "conditional", cfg)
