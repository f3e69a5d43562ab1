"""MI355X-native drop-in for doppel-speller's candidate-generation-and-scoring hot path.

Public surface (mirrors the reference, doppelspeller/match_maker.py and doppelspeller/feature_engineering.py):

    MatchMaker(data, truth_data, top_n).get_closest_matches(row_number)   -> list of title_id
    construct_features(title_number_of_characters, truth_number_of_characters, title, title_truth,
                       truth_words_counts, space_code, number_of_truth_titles, dummy, response)   (in place)
    FEATURES_COUNT, encode_title, get_truth_words_counts
    Prediction(truth_titles, truth_title_ids, model).generate_test_predictions(titles)   -> final_output (predict.py)
        .ranked_matches(titles, n)   -> the best n candidates per title in order, with scores (this project's own)
        .exhaustive_matches(titles, n)   -> the best n rows of the WHOLE truth set per title by the model alone, and
            where the Jaccard top_n put each of them (this project's own: tells a miss of the candidate stage from a
            miss of the model); closest_search_single_title(title, exhaustive=True) answers from it
        .evaluate(titles, actual_title_ids)   -> the counts of get-predictions-accuracy (cli.py) and custom_error
        .threshold_sweep(titles, actual_title_ids, levenshtein_thresholds, probability_thresholds)   -> those counts
            for every pair of the two thresholds, from one scoring pass (this project's own); with n_boot=, groups=,
            seed= also `sweep_bootstrap` (SweepBootstrap): every cell under one paired bootstrap of the titles, resampled
            on the device: frame() with an interval and share_best per cell, against(cell), best();
            validate_sweep_bootstrap(...) says what is accepted
        .duplicate_groups(levenshtein_threshold, probability_threshold)   -> the groups of truth titles that are
            duplicates of each other: the connected components of the exact, close and model links among the truth
            set's own rows, found on the device (this project's own)
        .one_to_one_matches(titles, n)   -> one answer per title with every truth title given to one title at most: the
            stable matching of the titles' ranked slots, found on the device (this project's own; for linking one
            de-duplicated file against another)
        .explain(titles)   -> for every title its best candidate by the model and why: the contribution of each of
            the 66 features to that pair's margin (TreeSHAP, or Saabas), computed on the device (this project's own);
            FEATURE_NAMES names the columns, top_contributions(contributions, n) picks the largest per row
    predictions_accuracy(predicted_title_ids, actual_title_ids)   -> the same counts from two id arrays
    ForestModel.fit_cover(rows) / set_cover(cover) / predict_contributions(rows)   -> node cover and per-feature
        contributions of a model (xgboost's pred_contribs / approx_contribs)
    ForestTrainer().fit(features, target, eval_features, eval_target, **parameters)   -> ForestModel (train.py; the
        booster parameters by keyword: train.validate_parameters)
    FeatureEngineering(truth_titles, truth_title_ids, train_titles, train_title_ids)
        .generate_train_and_evaluation_data_sets()   -> (train, train_target, evaluation, evaluation_target)
    train_model(truth_titles, truth_title_ids, train_titles, train_title_ids)   -> model, feature importances, the
        evaluation error matrix (train.train_model: the two steps above in one call, the feature matrix kept in HBM)
    cross_validate(features, target, parameter_grid(max_depth=[4, 5], eta=[0.1, 0.3]), n_folds=5)   -> the out-of-fold
        custom error of every parameter set and round, the best set and its model refit on all rows; the K folds x P
        sets are boosters of one batch on the device (ForestTrainerBatch), sharing bins, launches and the host sync
    tune_model_parameters(truth_titles, truth_title_ids, train_titles, train_title_ids, parameters)   -> the same
        from raw titles, folds by train title, the feature matrix kept in HBM (this project's own)
    ForestTrainer.fit(..., eval_metrics=("auc", "logloss")), cross_validate(..., metrics=("auc",), select_by="auc")   ->
        the reference's per-round train-auc / evaluation-auc log and the objective's own loss, computed on the device from
        the margins; roc_auc(scores, target) / auc_counts(scores, target) for any score vector (this project's own)
    ForestTrainer.fit(..., init_model=model), train_model(..., init_model=), cross_validate(..., init_model=),
        tune_model_parameters(..., init_model=)   -> continue boosting from an existing ForestModel (xgb.train's
        xgb_model=): k rounds continued for m more are exactly k + m rounds; `initial_error(s)` is the init model's own
        error; ForestModel.head(n) / extended(trees) cut and join forests (this project's own)
    FeatureEngineering.generate_hard_negatives(model, hard_n) / generate_device_hard_negatives   -> for every train title
        the wrong candidates the model likes best, scored and selected on the device; DeviceDataSets.
        with_hard_negatives(hard) appends them to the training matrix in HBM for fit_device(..., init_model=model)
        (this project's own)
    ForestTrainer.fit(..., sample_weight=w), ForestTrainerBatch.begin(..., sample_weight=w), cross_validate(...,
        sample_weight=w), train_model(..., kind_weights={"generated": 0.5, "positive": 2}), tune_model_parameters(...,
        kind_weights=)   -> per-row weights in the objective (xgb.DMatrix(weight=...)): a row's gradient and hessian times
        its weight, on the device; cuts, subsample draws, errors, metrics and cover stay unweighted;
        validate_sample_weight(w, n, beta) says what is accepted, kind_weights(rows, weights) weighs a training set's
        rows by their kind (this project's own)
    ForestTrainer.fit(..., monotone_constraints=c), ForestTrainerBatch.begin(..., monotone_constraints=c),
        cross_validate(..., monotone_constraints=c), train_model(..., monotone_constraints=ratio_constraints()),
        tune_model_parameters(..., monotone_constraints=)   -> a sign per feature (xgboost's monotone_constraints): the
        margin never falls (+1) or never rises (-1) as that feature rises, enforced in the split choice on the device;
        RATIO_FEATURE_NAMES are the 17 similarity ratios, ForestModel.monotone_violations(c) counts the splits of any
        model that break c, validate_monotone_constraints(c, n_features, names) says what is accepted (this project's own)
    ForestModel.permutation_importance(rows, target, n_repeats=5), permutation_importance_device(d_rows, n, d_target),
        train_model(..., permutation_repeats=5)   -> how much the evaluation error fn + beta * fp grows when a feature's
        column is shuffled (PermutationImportance: importance, importance_std, margin_shift, frame()); ForestModel.
        partial_dependence(rows, "title_ratio"), partial_dependence_device(...)   -> the mean margin along one feature
        (PartialDependence); both are one launch over a matrix staged once, integer sums, the same bits run after run;
        validate_inspection(...) says what is accepted (this project's own)
    ForestModel.refresh(features, target, eval_features, eval_target, eta=, reg_lambda=, beta=, sample_weight=),
        refresh_device(d_rows, n, target, ...), refresh_model(truth_titles, truth_title_ids, train_titles,
        train_title_ids, model)   -> keep every split of a trained model and re-estimate its leaves on new rows, tree by
        tree on the device (xgboost's updater="refresh"): RefreshResult with the new model, the exact gradient and
        hessian sums per node, cover, the gain of every split on that data, gain_importance() and the evaluation error
        per tree prefix; a model refreshed on its own training data comes back bit for bit; validate_refresh(...) says
        what is accepted (this project's own)
    compare_models([a, b], rows, target, groups=), compare_models_device(models, d_rows, n, d_target),
        bootstrap_accuracy({"a": ids_a, "b": ids_b}, actual_title_ids, groups=), train_model(..., bootstrap_repeats=2000)
        -> is model B better: the evaluation error of 1 to 64 models (or sets of predicted ids) over the same rows under
        one paired bootstrap, resampled by group on the device (ErrorBootstrap: errors, interval(), standard_error,
        difference(a, b) with its interval and share_better, frame()); bootstrap_counts(codes, groups) for any outcome
        codes; integer counts, the same bits run after run; validate_bootstrap(...) says what is accepted (this
        project's own)
    ForestModel.calibrate(rows, target), calibrate_device(d_rows, n, d_target), fit_isotonic(scores, target),
        train_model(..., calibrate=True), Prediction(..., calibrator=c)   -> what the probability means: the isotonic fit
        of the labels on the model's probability, on the device on exact integers (Calibrator: lo, hi, pos, neg, values,
        transform(), transform_device(), raw_threshold(q) for a probability_threshold at a calibrated level, frame(),
        save() / load()); a `calibrated_probability` column in ranked_matches, exhaustive_matches and explain;
        reliability(probabilities, target, n_bins) -> ReliabilityReport (counts, frame(), ece, mce, brier);
        validate_calibration(...) says what is accepted (this project's own)
    generate_misspelled_names(titles, seed)   -> generate_misspelled_name of every title (feature_engineering_prepare.py)
    edit_operations(truth_titles, titles)   -> which characters differ between a title and its match: the edit script of
        every pair (EditScripts: distance, ops, lengths, frame(), render(i)), aligned on the device one wave per pair;
        fit_misspelling_profile(truth_titles, titles, max_edits=4), FeatureEngineering.fit_misspelling_profile()   -> what
        kinds of errors labelled pairs hold (MisspellingProfile: edits_per_title(), operation_shares(), keyboard_share(),
        frame(), merged(), save() / load()); generate_misspelled_names(..., profile=p), FeatureEngineering(...,
        misspelling_profile=p), train_model / tune_model_parameters / refresh_model(..., misspelling_profile=p or "fit")
        -> generated rows that follow the data's own error model; validate_misspelling_profile(p) says what is accepted
        (this project's own)

All arithmetic runs in hand-written HIP kernels (csrc/*.hip -> libdoppel_amd.so, C ABI in include/doppel_amd.h);
there is no CPU fallback -- importing works without the library, calling anything that computes does not.
"""
from . import _lib  # noqa: F401
from ._lib import DoppelError, build_library, library_path  # noqa: F401
from .feature_engineering import (  # noqa: F401
    FEATURES_COUNT, FEATURE_NAMES, RATIO_FEATURE_NAMES, ratio_constraints, TitleTable, construct_features, construct_features_indexed, encode_title, encode_titles,
    get_truth_words_counts, levenshtein_ratio_batch, find_close_matches, exact_matches, ALLOWED_CHARACTERS, SPACE_CODE, SORT_KEY)
from .match_maker import MatchMaker, NativeProblem, TruthIndex  # noqa: F401
from .pipeline import CandidatePipeline  # noqa: F401
from .forest import (ForestModel, PartialDependence, PermutationImportance, RefreshResult, quantile_grid,  # noqa: F401
                     split_gains, validate_cover, validate_inspection, validate_refresh)
from .prediction import (ASSIGNMENT_COLUMNS, ASSIGNMENT_COUNTS, DUPLICATE_COLUMNS, EXHAUSTIVE_COLUMNS,  # noqa: F401
                         LINK_COLUMNS, RANKED_COLUMNS, SWEEP_COLUMNS, EXPLAIN_COLUMNS, Candidates, Prediction,
                         assignment_frame, duplicate_frame, predictions_accuracy, top_contributions,
                         validate_assignment, validate_duplicates, validate_exhaustive, validate_rank, validate_sweep)
from .training_set import (DeviceDataSets, DeviceHardNegatives, FeatureEngineering, generate_misspelled_names,  # noqa: F401
                           kind_weights, validate_hard)
from .train import (ForestTrainer, TrainModelResult, auc_counts, compute_cuts, compute_cuts_device,  # noqa: F401
                    evaluation_error_matrix, refresh_model, roc_auc, train_model, validate_init_model,
                    validate_monotone_constraints, validate_sample_weight)
from .tuning import (CrossValidation, ForestTrainerBatch, cross_validate, fold_assignment, parameter_grid,  # noqa: F401
                     select_parameters, tune_model_parameters)
from .bootstrap import (BootstrapCounts, ErrorBootstrap, ErrorDifference, SweepBootstrap, bootstrap_accuracy,  # noqa: F401
                        bootstrap_counts, compare_models, compare_models_device, validate_bootstrap,
                        validate_sweep_bootstrap)
from .calibration import (Calibrator, IsotonicFit, ReliabilityReport, fit_isotonic, fit_isotonic_device,  # noqa: F401
                          reliability, reliability_device, validate_calibration)
from .edits import (EditScripts, MisspellingProfile, edit_operations, fit_misspelling_profile,  # noqa: F401
                    validate_misspelling_profile)
from .text import transform_title, transform_titles  # noqa: F401
