"""The reference's personal-recommendation flow as a host helper over K4.

RecommenderSystem.py:227-249, restated for the MI355X engine:

  R:229  myUnratedMoviesRDD  = every (user, MovieID) of moviesRDD the user has not rated
  R:232  predictAll(...)     -> K4 als_predict on the device (inner join: movies the
                                model has never seen are dropped, as Spark's join does)
  R:236  movieCountsRDD      = (MovieID, number of ratings) from getCountsAndAverages
  R:242-245 join with counts and titles, keep NumRating > 75
  R:247  takeOrdered(20, key=-prediction)

`highest_rated_movies` is the script's first part (R:49-86) on the device (K16).
`movie_counts_and_averages` is R:50-58's getCountsAndAverages over the full ratings
(the count the R:245 filter reads).  Ties in the prediction keep moviesRDD order
(takeOrdered is heapq.nsmallest over the partitions: stable for equal keys).
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np

__all__ = ["movie_counts_and_averages", "highest_rated_movies", "personal_recommendations",
           "personal_recommendations_fold_in", "personal_recommendations_update",
           "personal_explanations", "similar_movies", "also_rated_movies"]


def movie_counts_and_averages(ratings) -> Dict[int, Tuple[int, float]]:
    """R:50-58 getCountsAndAverages over (user, movie, rating) triples:
    MovieID -> (number of ratings, average rating)."""
    from ._data import columns_of
    _, m, r = columns_of(ratings, ("user", "movie", "rating"))
    m = np.asarray(m, np.int64)
    r = np.asarray(r, np.float64)
    ids, inv, cnt = np.unique(m, return_inverse=True, return_counts=True)
    tot = np.bincount(inv, weights=r)
    return {int(a): (int(c), float(t) / int(c)) for a, c, t in zip(ids, cnt, tot)}


def highest_rated_movies(source, movies: Iterable[Sequence], min_count: int = 500,
                         num: int = 20) -> List[Tuple[float, str, int]]:
    """R:75-86, "movies with highest average rating and more than 500 reviews": (average
    rating, movie name, number of ratings) of the `num` movies of `movies` with MORE than
    `min_count` ratings, highest average first, equal averages by ascending MovieID.  Counts
    and sums come from one sweep of the item-side ratings on the device (K16,
    ALSCore.top_rated).

    source: a fitted model (MatrixFactorizationModel / ALSModel), an ALSCore, or raw (user,
            movie, rating) triples, from which an engine is built
    movies: (MovieID, title) pairs (moviesRDD, R:39); a rated movie without a title is left
            out, as R:71's join does."""
    from . import engine as _engine
    if isinstance(source, _engine.ALSCore):
        eng = source
    elif getattr(source, "engine", None) is not None:
        eng = source.engine
    else:
        from ._data import check_integers, columns_of, to_float32
        u, m, r = columns_of(source, ("user", "movie", "rating"))
        eng = _engine.ALSCore(check_integers(u, "user"), check_integers(m, "movie"),
                              to_float32(r))
    titles = {}
    for m, t in movies:
        titles.setdefault(int(m), str(t))
    ids, means, counts = (x.cpu().numpy() for x in eng.top_rated(eng.n_items, int(min_count)))
    out = [(float(a), titles[int(m)], int(c)) for m, a, c in zip(ids, means, counts)
           if int(m) in titles]
    return out[:int(num)]


def _engine_of(model):
    eng = getattr(model, "engine", None)
    if eng is None:
        raise TypeError("expected a MatrixFactorizationModel or ALSModel")
    return eng


def personal_recommendations_fold_in(model, rated: Iterable[Sequence], movies: Iterable[Sequence],
                                     counts, reg: float, min_count: int = 75, num: int = 20,
                                     trade_off=None) -> List[Tuple[float, str, int]]:
    """personal_recommendations' output — (predicted rating, movie name, number of
    ratings), highest prediction first — for a user who is NOT in the model, without the
    retrain of R:218: the user's factor row is folded in from `rated` against the fixed
    movie factors (K7) and the list comes from one filtered top-k (K5) whose candidates
    are the movies of `movies` with more than `min_count` ratings (R:245), the user's own
    rated movies excluded (R:229).

    rated:  the new user's (user, movie, rating) triples (one user id throughout)
    reg:    the lambda the model was trained with (explicit feedback, as the reference)
    movies / counts: as personal_recommendations.
    trade_off: None = the list above.  A number in [0, 1]: the filtered list is taken
        min(256, max(4 num, 50)) deep and re-ranked by maximal marginal relevance (K14,
        engine.diversify_rows) down to `num`, in pick order: 1 keeps the order above, lower
        values trade predicted rating for variety among the movies' factors."""
    rated = [(int(u), int(m), float(r)) for u, m, r, *_ in rated]
    if len({u for u, _, _ in rated}) > 1:
        raise ValueError("rated must hold the ratings of one user")
    titles = {}
    for m, t in movies:
        titles.setdefault(int(m), str(t))

    def count_of(m):
        c = counts.get(m)
        return None if c is None else (int(c[0]) if isinstance(c, tuple) else int(c))

    cand = [m for m in titles if -(2 ** 31) <= m < 2 ** 31 and (count_of(m) or 0) > min_count]
    if not rated or not cand:
        return []
    u, m, r = (np.asarray(x) for x in zip(*rated))
    eng = _engine_of(model)
    depth = int(num) if trade_off is None else min(256, max(4 * int(num), 50))
    _, ids, sc = eng.recommend_new(
        u.astype(np.int32), m.astype(np.int32), r.astype(np.float32), depth, reg=float(reg),
        exclude_rated=True, candidates=np.asarray(cand, np.int32))
    if ids.shape[0] == 0:   # none of the rated movies is known to the model
        return []
    if trade_off is not None and ids.shape[1] > 0:
        from . import engine as _engine
        rows = eng.iidx.rows_of(ids).to(ids.dtype)
        rows[~sc.isfinite()] = -1   # (an open slot carries a placeholder id)
        idx, sc, _ = _engine.diversify_rows(rows, sc, eng.V, eng.n_items, eng.rank,
                                            min(int(num), int(ids.shape[1])), float(trade_off))
        ids = _engine.ids_of(eng.iidx.ids(), idx)
    ids, sc = ids.cpu().numpy()[0], sc.cpu().numpy()[0]
    return [(float(s), titles[int(a)], count_of(int(a))) for a, s in zip(ids, sc)
            if np.isfinite(s)]


def personal_explanations(model, rated: Iterable[Sequence], movies: Iterable[Sequence],
                          movie_ids: Iterable[int], reg: float, num: int = 10
                          ) -> List[Tuple[str, float, List[Tuple[str, float, float]]]]:
    """Why the fold-in person of personal_recommendations_fold_in is recommended what they
    are: for each movie of `movie_ids` the model knows, (movie name, predicted rating,
    [(rated movie name, the rating given, its contribution to the prediction), ...]), the
    `num` largest contributions first — "because you rated X 5 and Y 4".  The prediction is
    the one the fold-in serves (the same normal equations, K11) and is the sum of one
    contribution per rating in `rated`, listed or not.

    rated:  the person's (user, movie, rating) triples (one user id throughout)
    movies: (MovieID, title) pairs; a movie without a title is named by its id
    reg:    the lambda the model was trained with (explicit feedback, as the reference)."""
    rated = [(int(u), int(m), float(r)) for u, m, r, *_ in rated]
    if len({u for u, _, _ in rated}) > 1:
        raise ValueError("rated must hold the ratings of one user")
    titles = {}
    for m, t in movies:
        titles.setdefault(int(m), str(t))
    want = [int(m) for m in movie_ids if -(2 ** 31) <= int(m) < 2 ** 31]
    if not rated or not want:
        return []
    u, m, r = (np.asarray(x) for x in zip(*rated))
    ratings = (u.astype(np.int32), m.astype(np.int32), r.astype(np.float32))
    _, ii, sc, ids, rat, con, n = (x.cpu().numpy() for x in _engine_of(model).explain(
        np.full(len(want), u[0], np.int32), np.asarray(want, np.int32), int(num), reg=float(reg),
        ratings=ratings))
    name = lambda a: titles.get(int(a), str(int(a)))
    return [(name(ii[p]), float(sc[p]),
             [(name(a), float(b), float(c))
              for a, b, c in zip(ids[p, :n[p]], rat[p, :n[p]], con[p, :n[p]])])
            for p in range(len(ii)) if not np.isnan(sc[p])]


def similar_movies(model, movie_ids: Iterable[int], movies: Iterable[Sequence], num: int = 10,
                   min_ratings=None, ratings=None
                   ) -> List[Tuple[str, List[Tuple[str, float]]]]:
    """"Which movies are like this one?": for each movie of `movie_ids` the model knows
    (ascending id), (movie name, [(neighbour's name, similarity), ...]) — the `num` movies
    whose factors have the largest cosine with its own, most similar first (K12).

    movies: (MovieID, title) pairs; a movie without a title is named by its id
    min_ratings with ratings: neighbours are restricted to the movies with MORE than
        min_ratings ratings in `ratings` ((user, movie, rating) triples, counted by
        movie_counts_and_averages): the reference's R:245 "more than 75 ratings" filter
        applied to neighbours.  The queried movies themselves need not pass it."""
    titles = {}
    for m, t in movies:
        titles.setdefault(int(m), str(t))
    want = [int(m) for m in movie_ids if -(2 ** 31) <= int(m) < 2 ** 31]
    if not want:
        return []
    cand = None
    if min_ratings is not None:
        if ratings is None:
            raise ValueError("min_ratings needs ratings= to count from")
        counts = movie_counts_and_averages(ratings)
        cand = np.asarray([m for m, (c, _) in counts.items()
                           if c > min_ratings and -(2 ** 31) <= m < 2 ** 31], np.int32)
    keys, ids, sc = (x.cpu().numpy() for x in _engine_of(model).similar(
        np.asarray(want, np.int32), int(num), False, candidates=cand))
    name = lambda a: titles.get(int(a), str(int(a)))
    return [(name(k), [(name(a), float(s)) for a, s in zip(ri, rs) if np.isfinite(s)])
            for k, ri, rs in zip(keys, ids, sc)]


def also_rated_movies(model, movies: Iterable[Sequence], movie_id: int, num: int = 10,
                      min_ratings: int = 0, measure: str = "jaccard"
                      ) -> List[Tuple[float, str, int, int]]:
    """"People who rated this movie also rated": (score, movie name, raters in common, number
    of ratings) of the `num` movies that share the most raters with `movie_id` in the ratings
    the model was fitted on, strongest first (K19, ALSCore.co_rated: counted from the
    ratings, the factors are not used).

    movies: (MovieID, title) pairs; a movie without a title is named by its id
    min_ratings: only movies with MORE than min_ratings training ratings are listed (the
        reference's R:245 filter, applied to the neighbours as similar_movies applies it);
        the queried movie itself need not pass it
    measure: "count", "jaccard" or "cosine" of the two rater sets
    An unknown movie_id gives []."""
    titles = {}
    for m, t in movies:
        titles.setdefault(int(m), str(t))
    if not -(2 ** 31) <= int(movie_id) < 2 ** 31:
        return []
    eng = _engine_of(model)
    st = eng.rating_stats(user_side=False)
    ids, counts = st["ids"].cpu().numpy(), st["count"].cpu().numpy()
    n_of = dict(zip(ids.tolist(), counts.tolist()))
    cand = ids[counts > int(min_ratings)].astype(np.int32)
    keys, nb, sc, common = (x.cpu().numpy() for x in eng.co_rated(
        np.asarray([int(movie_id)], np.int32), int(num), False, measure=measure,
        candidates=cand))
    if len(keys) == 0:
        return []
    return [(float(s), titles.get(int(a), str(int(a))), int(c), int(n_of[int(a)]))
            for a, s, c in zip(nb[0], sc[0], common[0]) if c > 0]


def personal_recommendations_update(model, user_id: int, rated: Iterable[Sequence],
                                    movies: Iterable[Sequence], num: int = 20,
                                    min_ratings: int = 75, iterations: int = 2,
                                    replace: bool = False) -> List[Tuple[float, str, int]]:
    """R:207-247 without building the model again: the user's ratings are added to the
    model's own training data (K17, ALSCore.add_ratings), the model is refitted warm for
    `iterations` iterations from its current user factors (ALSCore.refit), and the list is
    personal_recommendations' — (predicted rating, movie name, number of ratings) of the
    user's top `num` unrated movies with more than `min_ratings` ratings.  The counts are
    the engine's own statistics (K16) after the merge, so the ratings just added count.
    THE MODEL IS CHANGED IN PLACE: it now knows the user.  replace=True: a rating of a movie
    the user had rated before takes the place of the stored one (K18, ALSCore.set_ratings)
    instead of standing beside it — the call to make when the user comes back and changes
    their mind.

    rated:  the user's (user, movie, rating) triples (myRatedMovies, R:190-202), all of
            `user_id`
    movies: (MovieID, title) pairs (moviesRDD, R:39)."""
    rated = [(int(u), int(m), float(r)) for u, m, r, *_ in rated]
    if any(u != int(user_id) for u, _, _ in rated):
        raise ValueError("rated must hold the ratings of user_id")
    eng = _engine_of(model)
    if rated:
        u, m, r = (np.asarray(x) for x in zip(*rated))
        change = eng.set_ratings if replace else eng.add_ratings
        change(u.astype(np.int32), m.astype(np.int32), r.astype(np.float32))
        eng.refit(int(iterations))
    stats = eng.rating_stats(user_side=False)
    counts = dict(zip(stats["ids"].cpu().numpy().tolist(),
                      stats["count"].cpu().numpy().astype(np.int64).tolist()))
    return personal_recommendations(model, user_id, rated, movies, counts,
                                    min_count=int(min_ratings), num=int(num))


def personal_recommendations(model, user_id: int, rated: Iterable[Sequence],
                             movies: Iterable[Sequence], counts, min_count: int = 75,
                             num: int = 20) -> List[Tuple[float, str, int]]:
    """(predicted rating, movie name, number of ratings) for the user's top `num`
    unrated movies with more than `min_count` ratings, highest prediction first.

    rated:  the user's (user, movie, rating) triples (myRatedMovies, R:190-202)
    movies: (MovieID, title) pairs (moviesRDD, R:39)
    counts: MovieID -> number of ratings, or MovieID -> (count, average) as
            returned by movie_counts_and_averages (movieCountsRDD, R:236)."""
    rated_pairs = {(int(u), int(m)) for u, m, *_ in rated}
    movies = [(int(m), str(t)) for m, t in movies]
    cand = [(m, t) for m, t in movies if (int(user_id), m) not in rated_pairs]   # R:229
    if not cand:
        return []
    mids = np.fromiter((m for m, _ in cand), dtype=np.int64, count=len(cand))
    ok_range = (mids >= -(2 ** 31)) & (mids < 2 ** 31)
    pred = np.full(len(cand), np.nan)
    users = np.full(int(ok_range.sum()), int(user_id), np.int32)
    pred[ok_range] = _engine_of(model).predict(users, mids[ok_range].astype(np.int32)
                                               ).cpu().numpy()                  # R:232
    out = []
    for (m, title), p in zip(cand, pred):
        if np.isnan(p):           # predictAll's inner join drops unknown movies
            continue
        c = counts.get(m)         # R:242 join with movieCountsRDD
        if c is None:
            continue
        n = int(c[0]) if isinstance(c, tuple) else int(c)
        if n > min_count:         # R:245
            out.append((float(p), title, n))
    # R:247 takeOrdered(num, key=-rating): stable for equal predictions
    order = sorted(range(len(out)), key=lambda j: -out[j][0])
    return [out[j] for j in order[:num]]
