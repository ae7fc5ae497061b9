"""The PLDA stage end to end on a generated speaker corpus with known speaker means (40 speakers × 6 utterances, D = 16):
train, adapt, load the speakers, classify — the device chain against the same chain on the host twins, index for index, and
against the host specification (the direct formula); the batched ``Plda.pairwise`` against ``log_likelihood`` pair by pair;
``plda_knn`` against a sort of the host matrix; ``IvectorTrainer.compute_plda``'s file."""
import numpy as np
import pytest

from montreal_forced_aligner_amd import kalpy_api as K
from montreal_forced_aligner_amd import plda as P
from montreal_forced_aligner_amd.stats import plda_knn, plda_transform
from tests import plda_ref as R

pytestmark = pytest.mark.gpu

SPEAKERS, UTTS, D = 40, 6, 16


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """Speaker means far apart against the within-speaker spread (so the labels are unambiguous), vectors in an arbitrary
    affine frame; the model trained on half of every speaker's utterances, adapted on all vectors, written to a file."""
    rng = np.random.default_rng(11)
    frame = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    means = rng.standard_normal((SPEAKERS, D)) * 3.0
    vecs = (means[:, None, :] + rng.standard_normal((SPEAKERS, UTTS, D))) @ frame.T + 5.0
    ivectors = {f"s{s:02d}-u{u}": vecs[s, u] for s in range(SPEAKERS) for u in range(UTTS)}
    utt2spk = {k: k.split("-")[0] for k in ivectors}
    train = {k: v for k, v in ivectors.items() if int(k[-1]) < 3}
    model = P.train_plda(train, utt2spk)
    ad = P.PldaUnsupervisedAdaptor()
    ad.add_stats(1.0, P.normalize_length(np.stack(list(ivectors.values()))))
    model = ad.update_plda(model)
    path = tmp_path_factory.mktemp("plda") / "plda"
    model.write(path)
    spk_means = [(f"s{s:02d}", vecs[s, :3].mean(axis=0)) for s in range(SPEAKERS)]
    counts = {f"s{s:02d}": 3 for s in range(SPEAKERS)}
    test = P.normalize_length(np.stack([vecs[s, u] for s in range(SPEAKERS) for u in range(3, UTTS)]))
    labels = np.repeat(np.arange(SPEAKERS), UTTS - 3)
    return dict(path=path, model=model, spk_means=spk_means, counts=counts, test=test, labels=labels, ivectors=ivectors, utt2spk=utt2spk)


def test_classification_device_equals_host_and_labels_the_corpus(engine, corpus):
    dev, host = K.PldaScorer(corpus["path"]), K.PldaScorer(corpus["path"], backend="host")
    for s in (dev, host):
        s.load_speaker_ivectors(corpus["spk_means"], corpus["counts"])
    np.testing.assert_allclose(dev.speaker_ivectors, host.speaker_ivectors, rtol=1e-12, atol=1e-13)
    di, ds = dev.classify_speakers(corpus["test"])
    hi, hs = host.classify_speakers(corpus["test"])
    assert di.tolist() == hi.tolist()
    assert (np.abs(ds - hs) <= 2 * R.error_bound(corpus["model"].psi, host.speaker_ivectors, host.num_speaker_examples,
                                                 host._transform(corpus["test"])).max(axis=1)).all()
    # the host specification: the direct formula on the host's transformed vectors, pair by pair
    model = corpus["model"]
    spec = model.log_likelihood_ratios(host.speaker_ivectors, host.num_speaker_examples, model.transform_ivector(corpus["test"]))
    assert di.tolist() == spec.argmax(axis=1).tolist()
    assert (di == corpus["labels"]).mean() >= 0.95, (di == corpus["labels"]).mean()
    one = dev.classify_speaker(corpus["test"][7])
    assert one[0] == di[7] and one[1] == pytest.approx(ds[7], rel=1e-12)


def test_pairwise_against_log_likelihood_pair_by_pair(engine, corpus):
    plda = K.Plda.read(corpus["path"])
    x = plda.transform_ivectors(corpus["test"][:50])
    np.testing.assert_allclose(x, plda.transform_ivector(corpus["test"][:50]), rtol=1e-12, atol=1e-13)
    n = np.where(np.arange(50) % 3 == 0, 4, 1).astype(np.int32)
    mat = plda.pairwise(x, x, n)
    bound = R.error_bound(plda.model.psi, x, n, x)
    R.check_case(plda.model.psi, x, n, x)
    ref = R.llr(plda.model.psi, x, n, x)
    assert (np.abs(np.asarray(R.LD(mat) - ref, dtype=np.float64)) <= bound).all()
    own = R.direct_form_error(plda.model.psi, x, n, x)       # log_likelihood is float64 numpy: its own rounding beside the bound
    for i in range(0, 50, 7):
        for j in range(50):
            assert abs(mat[i, j] - plda.log_likelihood(x[j], int(n[j]), x[i])) <= bound[i, j] + own[i, j], (i, j)
    np.testing.assert_array_equal(plda.log_likelihood_distance_vectorized(x, x[3], n), -mat[3])
    assert plda.distance(x[2], x[3], 4) == -plda.log_likelihood(x[2], 4, x[3])


def test_knn_kth_distances_against_a_sorted_host_matrix(engine, corpus):
    model = corpus["model"]
    x = plda_transform(engine, model, corpus["test"])
    xh = x.cpu().numpy()
    host = model.log_likelihood_ratios(xh, 1, xh)
    np.fill_diagonal(host, -np.inf)
    k = 5
    idx, score = (t.cpu().numpy() for t in plda_knn(engine, model, x, x, k, exclude_diagonal=True))
    kth = -np.sort(-host, axis=1)[:, :k]
    # the k-th largest of two matrices that differ by at most e entrywise differ by at most e: the device's bound plus the
    # float64 host matrix's own rounding, the row's largest of each
    bound = (R.error_bound(model.psi, xh, 1, xh) + R.direct_form_error(model.psi, xh, 1, xh)).max(axis=1, keepdims=True)
    R.check_case(model.psi, xh, 1, xh)
    assert (np.abs(score - kth) <= bound).all()
    assert (idx != np.arange(idx.shape[0])[:, None]).all()
    ni, ns = K.Plda(model).nearest(xh, k)
    assert ni.tolist() == idx.tolist() and ns.tolist() == score.tolist()
    # most of an utterance's neighbours are its own speaker's other test utterances (two of them exist)
    same = corpus["labels"][idx[:, :2]] == corpus["labels"][:, None]
    assert same.mean() >= 0.9


def test_compute_plda_writes_a_model_that_reloads(corpus, tmp_path):
    from montreal_forced_aligner_amd.train import IvectorTrainer
    trainer = IvectorTrainer(backend=object())
    model = trainer.compute_plda(corpus["ivectors"], corpus["utt2spk"], directory=tmp_path)
    back = P.PldaModel.read(tmp_path / "plda")
    assert back.mean.tolist() == model.mean.tolist() and back.transform.tolist() == model.transform.tolist()
    assert back.psi.tolist() == model.psi.tolist() and (np.diff(back.psi) <= 0).all()
    again = P.train_plda(corpus["ivectors"], corpus["utt2spk"])
    assert again.psi.tolist() == model.psi.tolist()
    with pytest.raises(P.PldaTrainingError):
        trainer.compute_plda(corpus["ivectors"], {k: k for k in corpus["ivectors"]})
