"""Host-side classification metrics in NumPy, standing in for the three scikit-learn calls of the reference's
Fine-tuning/Classification/train.py (`roc_auc_score` :65-71, `simple_accuracy` :74-77, `metrics.confusion_matrix` :250,341)."""
import numpy as np


def rankdata_average(a):
    """1-based ranks of a 1-D array, ties sharing the average of the ranks they span."""
    a = np.asarray(a)
    order = np.argsort(a, kind="mergesort")
    s = a[order]
    first = np.r_[True, s[1:] != s[:-1]]              # start of each run of equal values
    starts = np.flatnonzero(first)
    ends = np.r_[starts[1:], len(s)]
    avg = (starts + 1 + ends) / 2.0                    # mean of ranks starts+1 .. ends
    ranks = np.empty(len(s), dtype=np.float64)
    ranks[order] = avg[np.cumsum(first) - 1]
    return ranks


def binary_auroc(labels, scores):
    """Area under the ROC curve of one class by ranks (the Mann-Whitney U statistic: concordant pairs + half the tied ones, over
    positive x negative pairs).  NaN when `labels` holds one value only."""
    y = np.asarray(labels).reshape(-1) > 0.5
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    npos = int(y.sum())
    nneg = y.size - npos
    if npos == 0 or nneg == 0:
        return float("nan")
    r = rankdata_average(s)
    return float((r[y].sum() - npos * (npos + 1) / 2.0) / (npos * float(nneg)))


def auroc_per_class(scores, labels):
    """scores, labels [N, C] -> list of C AUROCs (train.py:65-71); NaN for a class with one label value only."""
    scores, labels = np.asarray(scores), np.asarray(labels)
    if scores.ndim == 1:
        scores, labels = scores[:, None], labels.reshape(-1, 1)
    return [binary_auroc(labels[:, i], scores[:, i]) for i in range(scores.shape[1])]


def mean_auroc(aurocs, log=print):
    """Mean over the classes that have an AUROC; the others are left out with a message (scikit-learn raises there, which ends the
    reference's run on a small validation list).  NaN if no class has one."""
    skipped = [i for i, a in enumerate(aurocs) if np.isnan(a)]
    if skipped and log is not None:
        log("AUROC undefined for class(es) %s (one label value only): left out of the mean" % ", ".join(str(i) for i in skipped))
    kept = [a for a in aurocs if not np.isnan(a)]
    return float(np.mean(kept)) if kept else float("nan")


def simple_accuracy(preds, labels):
    """train.py:74-77: the mean of elementwise agreement."""
    return float(((np.asarray(preds) == np.asarray(labels)) * 1).mean())


def confusion_matrix(labels, preds, num_classes=None):
    """[num_classes, num_classes] int64, rows = true class, columns = predicted class (sklearn.metrics.confusion_matrix's layout)."""
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    preds = np.asarray(preds).reshape(-1).astype(np.int64)
    n = int(num_classes) if num_classes is not None else int(max(labels.max(initial=0), preds.max(initial=0))) + 1
    cm = np.zeros((n, n), dtype=np.int64)
    np.add.at(cm, (labels, preds), 1)
    return cm
