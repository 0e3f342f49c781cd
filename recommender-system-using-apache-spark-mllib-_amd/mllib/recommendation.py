"""pyspark.mllib.recommendation-compatible facade: ALS.train / trainImplicit,
MatrixFactorizationModel, Rating.

This is the surface the reference script actually calls
(``from pyspark.mllib.recommendation import ALS`` at RecommenderSystem.py:132;
``ALS.train(trainingRDD, rank, seed=seed, iterations=iterations,
lambda_=regularizationParameter)`` at :148-149, :163, :218;
``model.predictAll(pairsRDD)`` at :150, :165, :222, :232).  Each call maps 1:1:
RDDs become Python iterables / numpy arrays / pandas frames / torch tensors,
and the arithmetic runs on the MI355X engine.

Semantics kept from upstream pyspark/mllib (``mllib/recommendation.py``,
``MatrixFactorizationModel.scala``):
  * ratings are (user, product, rating) triples; ratings cast to float32;
  * ``predictAll`` is an inner join: pairs with an unknown user or product are
    dropped; predictions are fp64 dots of the fp32 factors (``ddot``);
  * ``lambda_`` default 0.01, ``iterations`` default 5, ``blocks`` ignored
    (single CSR per side), ``nonnegative=True`` is out of scope.
"""
from __future__ import annotations

import zlib
from collections import namedtuple
from typing import Iterable, List, Optional

import numpy as np

from .. import engine as _engine
from .._data import check_integers, columns_of, to_float32

__all__ = ["ALS", "BaselineModel", "MatrixFactorizationModel", "Rating"]

_DEFAULT_SEED = zlib.crc32(b"org.apache.spark.mllib.recommendation.ALS")


class Rating(namedtuple("Rating", ["user", "product", "rating"])):
    """Represents a (user, product, rating) tuple (pyspark.mllib.recommendation.Rating)."""

    def __reduce__(self):
        return Rating, (int(self.user), int(self.product), float(self.rating))


def _triples(ratings):
    if hasattr(ratings, "columns") and {"user", "product", "rating"} <= set(ratings.columns):
        cols = ("user", "product", "rating")
        u, i, r = columns_of(ratings, cols)
    elif hasattr(ratings, "columns"):  # any 3-column frame, positional
        u, i, r = columns_of(ratings.to_numpy(), ("user", "product", "rating"))
    else:
        u, i, r = columns_of(ratings, ("user", "product", "rating"))
    return check_integers(u, "user"), check_integers(i, "product"), to_float32(r)


def _check_mode(mode, iterations) -> None:
    if mode not in ("refit", "refresh", "none"):
        raise ValueError(f"mode must be 'refit', 'refresh' or 'none', got {mode!r}")
    if int(iterations) < 0:
        raise ValueError(f"iterations must be >= 0, got {iterations}")


def _pairs(user_product):
    if hasattr(user_product, "to_numpy"):
        user_product = user_product.to_numpy()
    u, i = columns_of(user_product, ("user", "product"))
    return check_integers(u, "user"), check_integers(i, "product")


class MatrixFactorizationModel:
    """A matrix factorisation model trained by ALS; factors stay in HBM."""

    def __init__(self, core: "_engine.ALSCore"):
        self._core = core

    @property
    def rank(self) -> int:
        return self._core.rank

    @property
    def engine(self) -> "_engine.ALSCore":
        return self._core

    def predict(self, user: int, product: int) -> float:
        p = self._core.predict(np.array([user], np.int32), np.array([product], np.int32))
        v = float(p.cpu().numpy()[0])
        if np.isnan(v):
            raise KeyError(f"unknown user {user} or product {product}")
        return v

    def predictAll(self, user_product) -> List[Rating]:
        """Predicted Ratings for the (user, product) pairs whose ids are both known
        (inner join, as MatrixFactorizationModel.predict(RDD) does)."""
        u, i = _pairs(user_product)
        if len(u) == 0:
            return []
        p = self._core.predict(u, i).cpu().numpy()
        ok = ~np.isnan(p)
        return [Rating(int(a), int(b), float(c)) for a, b, c in zip(u[ok], i[ok], p[ok])]

    def predictAllArrays(self, users, products) -> np.ndarray:
        """fp64 predictions for arrays of ids (NaN where an id is unknown)."""
        return self._core.predict(check_integers(users, "user"),
                                  check_integers(products, "product")).cpu().numpy()

    def rmse(self, ratings) -> float:
        """computeError(predictAll(pairs), ratings) fused on the device (K4)."""
        u, i, r = _triples(ratings)
        rm, _ = self._core.rmse(u, i, r)
        return rm

    def regressionMetrics(self, ratings) -> dict:
        """pyspark.mllib.evaluation.RegressionMetrics of predictAll against held-out (user,
        product, rating) rows, fused on the device (K8): {"mse", "rmse", "mae", "r2", "var",
        "n", "dropped", "meanLabel", "varLabel"}.  Rows with an unknown user or product are
        left out and counted in "dropped" (predictAll's inner join)."""
        u, i, r = _triples(ratings)
        return self._core.regression_metrics(u, i, r)

    def _statistics(self, user_side: bool):
        st = self._core.rating_stats(user_side=user_side)
        ids, cnt, mean = (st[k].cpu().numpy() for k in ("ids", "count", "mean"))
        return [(int(a), int(c), float(m)) for a, c, m in zip(ids, cnt, mean)]

    def productStatistics(self):
        """[(product, number of ratings, average rating)] of the training ratings, ascending
        id — the reference's getCountsAndAverages (RecommenderSystem.py:50-66) in one sweep on
        the device (K16).  Raises ValueError on a loaded model, which holds no ratings."""
        return self._statistics(False)

    def userStatistics(self):
        """productStatistics for the users."""
        return self._statistics(True)

    def trainingObjective(self, lambda_: float, implicit: bool = False,
                          alpha: float = 0.01) -> dict:
        """The objective ALS minimises, of this model's factors on the ratings it was trained
        on (K10): {"objective", "data", "reg", "scale", "n", "n_positive"}.  lambda_ (and
        implicit / alpha, as in trainImplicit) are arguments because this model stores no
        training parameters.  Raises ValueError on a loaded model, which holds no ratings."""
        _check(self.rank, 0, lambda_, False, alpha)
        return self._core.objective(float(lambda_), bool(implicit), float(alpha))

    def rankingMetrics(self, ratings, k: int, *, threshold: Optional[float] = None,
                       exclude=None, candidates=None) -> dict:
        """Ranking quality of each user's top-k products against held-out (user,
        product[, rating]) rows: {"precision", "recall", "map", "ndcg", "hitRate", "rows"}
        with pyspark.mllib.evaluation.RankingMetrics' definitions at k, means over the
        users with at least one relevant row (rating >= threshold when given).  exclude /
        candidates as recommendProductsForUsers.  Lists and metrics stay on the device."""
        if threshold is not None:
            u, i, r = _triples(ratings)
        else:
            (u, i), r = _pairs(ratings), None
        return self._core.rank_metrics(u, i, int(k), ratings=r, threshold=threshold,
                                       **self._filters(exclude, candidates, True))

    def fullRankingMetrics(self, ratings, *, threshold: Optional[float] = None,
                           weighted: bool = False, exclude=None, candidates=None) -> dict:
        """Where held-out (user, product[, rating]) rows sit in each user's ordering of ALL
        admissible products: {"expectedPercentileRank" (0.5 = random, lower is better;
        rating-weighted with weighted=True, the measure of the implicit-ALS paper),
        "meanPercentileRank", "auc", "mrr", "rows", "pairs", "inadmissible", "dropped"}: what
        a trainImplicit model is judged by.  exclude / candidates as
        recommendProductsForUsers.  One sweep of the whole score matrix on the device (K9)."""
        if threshold is not None or weighted:
            u, i, r = _triples(ratings)
        else:
            (u, i), r = _pairs(ratings), None
        return self._core.full_rank_metrics(u, i, ratings=r, threshold=threshold,
                                            weighted=bool(weighted),
                                            **self._filters(exclude, candidates, True))

    def userFeatures(self):
        ids, F = self._core.user_factors()
        F = F.double().cpu().numpy()
        return [(int(a), tuple(row)) for a, row in zip(ids.cpu().numpy(), F)]

    def productFeatures(self):
        ids, F = self._core.item_factors()
        F = F.double().cpu().numpy()
        return [(int(a), tuple(row)) for a, row in zip(ids.cpu().numpy(), F)]

    def _filters(self, exclude, candidates, user_side):
        """exclude: None, "train" or (user, product[, rating]) rows never to list;
        candidates: ids of the listed side (products for users, users for products)."""
        if exclude is not None and not isinstance(exclude, str):
            u, i = _pairs(exclude)
            exclude = (u, i) if user_side else (i, u)
        if candidates is not None:
            candidates = check_integers(np.asarray(candidates).reshape(-1),
                                        "product" if user_side else "user")
        return dict(exclude=exclude, candidates=candidates)

    def _one(self, key, num, user_side, exclude=None, candidates=None):
        keys, ids, sc = self._core.recommend_subset(
            [int(key)], int(num), user_side, **self._filters(exclude, candidates, user_side))
        if keys.numel() == 0:
            raise KeyError(f"unknown id {key}")
        ids, sc = ids.cpu().numpy()[0], sc.cpu().numpy()[0]
        return [Rating(key, int(a), float(s)) if user_side else Rating(int(a), key, float(s))
                for a, s in zip(ids, sc) if np.isfinite(s)]

    def recommendProducts(self, user: int, num: int, *, exclude=None,
                          candidates=None) -> List[Rating]:
        """exclude="train" (or (user, product) rows) leaves those pairs out of the list;
        candidates= restricts the products listed (RecommenderSystem.py:229 / :245)."""
        return self._one(int(user), num, True, exclude, candidates)

    def recommendUsers(self, product: int, num: int, *, exclude=None,
                       candidates=None) -> List[Rating]:
        return self._one(int(product), num, False, exclude, candidates)

    def _similar_one(self, key, num, user_side, candidates):
        if candidates is not None:
            candidates = check_integers(np.asarray(candidates).reshape(-1),
                                        "user" if user_side else "product")
        keys, ids, sc = self._core.similar([int(key)], int(num), user_side,
                                           candidates=candidates)
        if keys.numel() == 0:
            raise KeyError(f"unknown id {key}")
        ids, sc = ids.cpu().numpy()[0], sc.cpu().numpy()[0]
        return [(int(a), float(s)) for a, s in zip(ids, sc) if np.isfinite(s)]

    def similarProducts(self, product: int, num: int, *, candidates=None):
        """The `num` products most like `product`: [(product, similarity)], the cosine of the
        product factors, most similar first (K12).  candidates= restricts the neighbours to
        those product ids.  The product itself is never listed; products whose factors are
        all zero or not finite are nobody's neighbour.  KeyError for an unknown product."""
        return self._similar_one(int(product), num, False, candidates)

    def similarUsers(self, user: int, num: int, *, candidates=None):
        """similarProducts among the user factors: [(user, similarity)]."""
        return self._similar_one(int(user), num, True, candidates)

    def _co_rated_one(self, key, num, user_side, measure, minCommon, candidates):
        if candidates is not None:
            candidates = check_integers(np.asarray(candidates).reshape(-1),
                                        "user" if user_side else "product")
        keys, ids, sc, common = self._core.co_rated([int(key)], int(num), user_side,
                                                    measure=measure, min_common=int(minCommon),
                                                    candidates=candidates)
        if keys.numel() == 0:
            raise KeyError(f"unknown id {key}")
        ids, sc, common = ids.cpu().numpy()[0], sc.cpu().numpy()[0], common.cpu().numpy()[0]
        return [(int(a), float(s), int(c)) for a, s, c in zip(ids, sc, common) if c > 0]

    def coRatedProducts(self, product: int, num: int, *, measure: str = "jaccard",
                        minCommon: int = 1, candidates=None):
        """"Who rated this also rated": the `num` products that share the most raters with
        `product` in the training ratings, [(product, score, common raters)], strongest first
        (K19; exact integer counts, the factors are not used).  measure: "count", "jaccard"
        or "cosine" of the two rater sets; a product is listed from minCommon shared raters
        and, with candidates=, only when it is among those ids.  KeyError for an unknown
        product; ValueError on a loaded model, which holds no ratings."""
        return self._co_rated_one(int(product), num, False, measure, minCommon, candidates)

    def coRatedUsers(self, user: int, num: int, *, measure: str = "jaccard", minCommon: int = 1,
                     candidates=None):
        """coRatedProducts among the users: [(user, score, products both rated)]."""
        return self._co_rated_one(int(user), num, True, measure, minCommon, candidates)

    def recommendProductsForUsers(self, num: int, *, exclude=None, candidates=None):
        keys, ids, sc = self._core.recommend_all(int(num), True,
                                                 **self._filters(exclude, candidates, True))
        keys, ids, sc = keys.cpu().numpy(), ids.cpu().numpy(), sc.cpu().numpy()
        return [(int(k), [Rating(int(k), int(a), float(s)) for a, s in zip(ri, rs)
                          if np.isfinite(s)])
                for k, ri, rs in zip(keys, ids, sc)]

    def recommendProductsDiverse(self, user: int, num: int, tradeOff: float = 0.7, *, pool=None,
                                 exclude=None, candidates=None):
        """recommendProducts re-ranked by maximal marginal relevance (K14): (list of Rating in
        pick order, intra-list similarity of the list).  The `pool` best products (None:
        min(256, max(4 num, 50))) are the candidates; each pick maximises tradeOff *
        relevance - (1 - tradeOff) * (largest cosine to the products already picked), so
        tradeOff = 1 is recommendProducts and lower values trade rating for variety.
        KeyError for an unknown user."""
        user = int(user)
        keys, ids, sc, ils = self._core.recommend_diverse(
            int(num), True, ids=[user], trade_off=float(tradeOff), pool=pool,
            **self._filters(exclude, candidates, True))
        if keys.numel() == 0:
            raise KeyError(f"unknown id {user}")
        ids, sc = ids.cpu().numpy()[0], sc.cpu().numpy()[0]
        return ([Rating(user, int(a), float(s)) for a, s in zip(ids, sc) if np.isfinite(s)],
                float(ils[0]))

    def recommendProductsForUsersDiverse(self, num: int, tradeOff: float = 0.7, *, pool=None,
                                         exclude=None, candidates=None):
        """recommendProductsDiverse for every user: [(user, list of Rating, intra-list
        similarity)]."""
        keys, ids, sc, ils = self._core.recommend_diverse(
            int(num), True, trade_off=float(tradeOff), pool=pool,
            **self._filters(exclude, candidates, True))
        keys, ids, sc, ils = (x.cpu().numpy() for x in (keys, ids, sc, ils))
        return [(int(k), [Rating(int(k), int(a), float(s)) for a, s in zip(ri, rs)
                          if np.isfinite(s)], float(v))
                for k, ri, rs, v in zip(keys, ids, sc, ils)]

    def listMetrics(self, num: int, *, exclude=None, candidates=None) -> dict:
        """Every user's top-`num` products looked at together (K15): {"coverage", "gini",
        "entropy", "effectiveItems", "personalization", "topItemShare", "novelty",
        "averagePopularity", "longTailShare", "lists", "entries", "skipped"} — how much of the
        catalogue the lists reach, how concentrated exposure is, how obscure the listed
        products are and how much two users' lists overlap (engine.list_metrics_dict).
        exclude / candidates as recommendProductsForUsers; candidates also defines the
        catalogue.  Lists and measures stay on the device.  A loaded model holds no rating
        counts: its three popularity fields are NaN."""
        return self._core.list_metrics(top=int(num), user_side=True,
                                       **self._filters(exclude, candidates, True))

    def foldInUsers(self, ratings, lambda_: float, *, implicit: bool = False,
                    alpha: float = 0.01, nonnegative: bool = False):
        """Factors for users that are not in the model, from their (user, product,
        rating) triples alone and without a refit: [(user, array)] in ascending user
        order, each solved against the fixed product factors (one row of one ALS
        half-sweep, K7).  lambda_ (and implicit / alpha, as in trainImplicit) are
        arguments because this model stores no training parameters.  Products the model
        does not know are skipped; the model itself is not changed.  nonnegative: solve
        each row under x >= 0 (K13), as ALS.trainNonnegative does."""
        _check(self.rank, 0, lambda_, False, alpha)
        u, i, r = _triples(ratings)
        extra = dict(nonnegative=True) if nonnegative else {}
        keys, X, _ = self._core.fold_in(u, i, r, reg=float(lambda_), implicit=bool(implicit),
                                        alpha=float(alpha), **extra)
        X = X.double().cpu().numpy()
        return [(int(a), row) for a, row in zip(keys.cpu().numpy(), X)]

    def recommendProductsForNewUsers(self, ratings, num: int, lambda_: float, *,
                                     implicit: bool = False, alpha: float = 0.01,
                                     exclude_rated: bool = True, candidates=None,
                                     nonnegative: bool = False):
        """Top `num` products for users that are not in the model (foldInUsers, then K5):
        [(user, [Rating])] as recommendProductsForUsers returns.  exclude_rated: a user's
        own rated products are left out; candidates: product ids the lists are restricted
        to.  Users without a single rating of a known product are absent.  nonnegative: as
        foldInUsers."""
        _check(self.rank, 0, lambda_, False, alpha)
        u, i, r = _triples(ratings)
        if candidates is not None:
            candidates = check_integers(np.asarray(candidates).reshape(-1), "product")
        extra = dict(nonnegative=True) if nonnegative else {}
        keys, ids, sc = self._core.recommend_new(
            u, i, r, int(num), reg=float(lambda_), implicit=bool(implicit), alpha=float(alpha),
            exclude_rated=bool(exclude_rated), candidates=candidates, **extra)
        keys, ids, sc = keys.cpu().numpy(), ids.cpu().numpy(), sc.cpu().numpy()
        return [(int(k), [Rating(int(k), int(a), float(s)) for a, s in zip(ri, rs)
                          if np.isfinite(s)])
                for k, ri, rs in zip(keys, ids, sc)]

    def explain(self, user_product, lambda_: float, num: int = 10, *, implicit: bool = False,
                alpha: float = 0.01, ratings=None):
        """Each (user, product) pair explained by the user's own ratings: [(user, product,
        score, [(product, rating, contribution), ...])], at most `num` (<= 32) contributions,
        largest first.  score is the sum of one contribution per rating of the user (all of
        them, listed or not): the user's factor solves normal equations that are linear in
        those ratings (K11).  lambda_ (and implicit / alpha, as in trainImplicit) are
        arguments because this model stores no training parameters.  ratings=None explains
        from the ratings the model was trained on; a loaded model holds none and needs
        ratings= — (user, product, rating) triples of the users to explain, who need not be
        in the model.  Pairs of users without ratings are absent; a product the model does
        not know gives NaN and no contributions."""
        _check(self.rank, 0, lambda_, False, alpha)
        u, i = _pairs(user_product)
        if ratings is not None:
            ratings = _triples(ratings)
        uu, ii, sc, ids, rat, con, n = (x.cpu().numpy() for x in self._core.explain(
            u, i, int(num), reg=float(lambda_), implicit=bool(implicit), alpha=float(alpha),
            ratings=ratings))
        return [(int(uu[r]), int(ii[r]), float(sc[r]),
                 [(int(a), float(b), float(c))
                  for a, b, c in zip(ids[r, :n[r]], rat[r, :n[r]], con[r, :n[r]])])
                for r in range(len(uu))]

    def update(self, ratings, iterations: int = 2, mode: str = "refit", replace: bool = False
               ) -> "MatrixFactorizationModel":
        """Add `ratings` (tuples or Ratings, as ALS.train takes them) to the model's training
        data and bring the factors up to date without training again — the reference's
        "add my ratings, train again" (RecommenderSystem.py:207-218) on the model it already
        has (K17, ALSCore.add_ratings).  THIS MODEL IS CHANGED IN PLACE and returned.
        mode: "refit" = `iterations` warm iterations over all rows from the current user
        features, with the lambda / implicit / alpha / solver it was trained with;
        "refresh" = only the users and products of `ratings` are solved again; "none" = the
        ratings are merged and new ids get fold-in features.  replace=True: a rating of a
        (user, product) pair the model already holds takes the place of every stored one
        instead of standing beside it, and of a pair that is several times in `ratings` the
        last counts (K18, ALSCore.set_ratings).  Not on a loaded model."""
        _check_mode(mode, iterations)
        u, i, r = _triples(ratings)
        if replace:
            self._core.set_ratings(u, i, r, seed=_DEFAULT_SEED)
        else:
            self._core.add_ratings(u, i, r, seed=_DEFAULT_SEED)
        return self._bring_up_to_date(mode, iterations)

    def _bring_up_to_date(self, mode, iterations) -> "MatrixFactorizationModel":
        if mode == "refit":
            self._core.refit(int(iterations))
        elif mode == "refresh":
            self._core.refresh()
        return self

    def remove(self, user_product, iterations: int = 2, mode: str = "refit"
               ) -> "MatrixFactorizationModel":
        """Take the ratings of the listed (user, product) pairs out of the model's training
        data — every stored rating of each pair — and bring the features up to date without
        training again (K18, ALSCore.remove_ratings).  THIS MODEL IS CHANGED IN PLACE and
        returned.  A user or product left without a rating leaves the model; a pair the
        model does not hold is ignored.  mode as in update(): "refit", "refresh" (only the
        users and products that lost a rating are solved again) or "none".  Not on a loaded
        model."""
        _check_mode(mode, iterations)
        self._core.remove_ratings(*_pairs(user_product))
        return self._bring_up_to_date(mode, iterations)

    def removeUsers(self, users, iterations: int = 2, mode: str = "refit"
                    ) -> "MatrixFactorizationModel":
        """remove() of every rating of the listed users: they leave the model, and so does a
        product only they had rated."""
        _check_mode(mode, iterations)
        self._core.remove_users(check_integers(np.asarray(list(users)), "user"))
        return self._bring_up_to_date(mode, iterations)

    def removeProducts(self, products, iterations: int = 2, mode: str = "refit"
                       ) -> "MatrixFactorizationModel":
        """remove() of every rating of the listed products."""
        _check_mode(mode, iterations)
        self._core.remove_items(check_integers(np.asarray(list(products)), "product"))
        return self._bring_up_to_date(mode, iterations)

    def save(self, sc, path: str, overwrite: bool = False) -> None:
        """MatrixFactorizationModel.save(sc, path) in Spark's layout (``sc`` is ignored)."""
        from .. import persistence
        uids, U = self._core.user_factors()
        pids, V = self._core.item_factors()
        persistence.save_mllib(path, self.rank, uids.cpu().numpy(), U.cpu().numpy(),
                               pids.cpu().numpy(), V.cpu().numpy(), overwrite=overwrite)

    @classmethod
    def load(cls, sc, path: str) -> "MatrixFactorizationModel":
        """MatrixFactorizationModel.load(sc, path): factors back into HBM (serving only)."""
        from .. import persistence
        _, uids, U, pids, V = persistence.load_mllib(path)
        return cls(_engine.ALSCore.from_factors(uids, U.astype(np.float32), pids,
                                                V.astype(np.float32)))

    def recommendUsersForProducts(self, num: int, *, exclude=None, candidates=None):
        keys, ids, sc = self._core.recommend_all(int(num), False,
                                                 **self._filters(exclude, candidates, False))
        keys, ids, sc = keys.cpu().numpy(), ids.cpu().numpy(), sc.cpu().numpy()
        return [(int(k), [Rating(int(a), int(k), float(s)) for a, s in zip(ri, rs)
                          if np.isfinite(s)])
                for k, ri, rs in zip(keys, ids, sc)]


def _check(rank, iterations, lambda_, nonnegative, alpha=0.0):
    if int(rank) < 1:
        raise ValueError(f"rank must be >= 1, got {rank}")
    if int(rank) > 128:
        raise NotImplementedError("rank > 128 is not supported by this build of the HIP kernels")
    if int(iterations) < 0:
        raise ValueError(f"iterations must be >= 0, got {iterations}")
    if lambda_ < 0:
        raise ValueError(f"lambda_ must be >= 0, got {lambda_}")
    if alpha < 0:
        raise ValueError(f"alpha must be >= 0, got {alpha}")
    if nonnegative:
        raise NotImplementedError(
            "the Spark parameter nonnegative=True is not wired to the NNLS solver yet: use "
            "ALS.trainNonnegative (K13), which trains the same nonnegative model")


class ALS:
    """Alternating Least Squares matrix factorisation (pyspark.mllib API)."""

    @classmethod
    def train(cls, ratings, rank: int, iterations: int = 5, lambda_: float = 0.01,
              blocks: int = -1, nonnegative: bool = False, seed: Optional[int] = None
              ) -> MatrixFactorizationModel:
        _check(rank, iterations, lambda_, nonnegative)
        u, i, r = _triples(ratings)
        core = _engine.make_engine(u, i, r)
        core.fit(int(rank), int(iterations), float(lambda_), False, 1.0,
                 seed=_DEFAULT_SEED if seed is None else int(seed))
        return MatrixFactorizationModel(core)

    @classmethod
    def trainHoldout(cls, ratings, rank: int, iterations: int = 5, lambda_: float = 0.01,
                     blocks: int = -1, nonnegative: bool = False, seed: Optional[int] = None,
                     holdOut: int = 1, splitSeed: Optional[int] = None):
        """train() under the leave-k-out protocol: `holdOut` ratings of every user are held
        out (holdOut=1: leave-one-out), chosen on the GPU from (splitSeed, user, product)
        (ALSCore.split, K20; no product leaves the training part), and the model is trained
        on the rest.  Returns (model, held): held is the list of held-out Rating rows, users
        ascending, a user's ratings in input order.  splitSeed None = seed.  Not a pyspark
        method."""
        _check(rank, iterations, lambda_, nonnegative)
        if isinstance(holdOut, bool) or int(holdOut) != holdOut or int(holdOut) < 1:
            raise ValueError(f"holdOut must be an integer >= 1, got {holdOut!r}")
        u, i, r = _triples(ratings)
        full = _engine.make_engine(u, i, r)
        if not isinstance(full, _engine.ALSCore):
            raise NotImplementedError("trainHoldout needs the single-GPU engine")
        seed = _DEFAULT_SEED if seed is None else int(seed)
        core, held = full.split(count=int(holdOut),
                                seed=seed if splitSeed is None else int(splitSeed))
        del full
        core.fit(int(rank), int(iterations), float(lambda_), False, 1.0, seed=seed)
        hu, hi, hr = (x.cpu().numpy().tolist() for x in held)
        return MatrixFactorizationModel(core), [Rating(*t) for t in zip(hu, hi, hr)]

    @classmethod
    def trainImplicit(cls, ratings, rank: int, iterations: int = 5, lambda_: float = 0.01,
                      blocks: int = -1, alpha: float = 0.01, nonnegative: bool = False,
                      seed: Optional[int] = None) -> MatrixFactorizationModel:
        _check(rank, iterations, lambda_, nonnegative, alpha)
        u, i, r = _triples(ratings)
        core = _engine.make_engine(u, i, r)
        core.fit(int(rank), int(iterations), float(lambda_), True, float(alpha),
                 seed=_DEFAULT_SEED if seed is None else int(seed))
        return MatrixFactorizationModel(core)


    @classmethod
    def trainNonnegative(cls, ratings, rank: int, iterations: int = 5, lambda_: float = 0.01,
                         seed: Optional[int] = None, implicitPrefs: bool = False,
                         alpha: float = 0.01) -> MatrixFactorizationModel:
        """train / trainImplicit with Spark's NNLSSolver in place of CholeskySolver — what
        `nonnegative=True` selects in Spark: every factor of the model is >= 0 (K13).  Not a
        pyspark method: the Spark spelling train(nonnegative=True) still raises."""
        _check(rank, iterations, lambda_, False, alpha)
        u, i, r = _triples(ratings)
        core = _engine.make_engine(u, i, r)
        core.fit(int(rank), int(iterations), float(lambda_), bool(implicitPrefs),
                 float(alpha) if implicitPrefs else 1.0,
                 seed=_DEFAULT_SEED if seed is None else int(seed), nonnegative=True)
        return MatrixFactorizationModel(core)


class BaselineModel:
    """The mean / damped-bias predictor mu + b_u + b_i of (user, product, rating) rows (K16,
    ALSCore.fit_baseline): what the reference's "Comparing your model" step
    (RecommenderSystem.py:172-177) measures a factor model against.  An id the training rows
    do not hold adds a zero bias, so every pair has a prediction."""

    def __init__(self, baseline: "_engine.Baseline"):
        self._base = baseline

    @classmethod
    def train(cls, ratings, method: str = "bias", regUser: float = 10.0, regItem: float = 25.0,
              iterations: int = 10) -> "BaselineModel":
        """method: "global" (the training mean), "item", "user" or "bias" (`iterations`
        alternating sweeps of the damped item and user biases)."""
        u, i, r = _triples(ratings)
        core = _engine.make_engine(u, i, r)
        return cls(core.fit_baseline(method, float(regUser), float(regItem), int(iterations)))

    @property
    def baseline(self) -> "_engine.Baseline":
        return self._base

    @property
    def globalMean(self) -> float:
        return self._base.mu

    def predict(self, user: int, product: int) -> float:
        p = self._base.predict(np.array([user], np.int32), np.array([product], np.int32))
        return float(p.cpu().numpy()[0])

    def predictAll(self, user_product) -> List[Rating]:
        """A Rating for every (user, product) pair, unknown ids included."""
        u, i = _pairs(user_product)
        if len(u) == 0:
            return []
        p = self._base.predict(u, i).cpu().numpy()
        return [Rating(int(a), int(b), float(c)) for a, b, c in zip(u, i, p)]

    def regressionMetrics(self, ratings) -> dict:
        """MatrixFactorizationModel.regressionMetrics' dict for the baseline; no row is
        dropped."""
        u, i, r = _triples(ratings)
        return self._base.regression_metrics(u, i, r)


def compute_error(predicted: Iterable, actual: Iterable) -> float:
    """RecommenderSystem.py:103-129 computeError as host glue over predictAll output:
    join on (user, product), sqrt(mean squared error).  (Use
    MatrixFactorizationModel.rmse for the fused on-device form.)"""
    import math
    pred = {}
    for u, i, r in predicted:
        pred.setdefault((int(u), int(i)), []).append(float(r))
    total, n = 0.0, 0
    for u, i, r in actual:
        for p in pred.get((int(u), int(i)), ()):
            total += (float(r) - p) ** 2
            n += 1
    return math.sqrt(total / n)
