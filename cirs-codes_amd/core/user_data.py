"""Assembly of the user-model training sets from the KuaiRec files (reference CIRS-UserModel-kuaishou.py:86-148,
`load_dataset_kuaishou`; DeepFM-IPS-pairwise.py:89-146, PD-pairwise.py:111-168 and DICE.py:77-182 for the debiasing baselines): positives from big_matrix.csv joined with the item categories, one sampled negative per row, the
exposure effect of every interaction; the two O(big) loops run on the device (core.util.negative_sampling,
core.util.compute_exposure_effect_kuaishouRec)."""
import json
import os

import numpy as np
import pandas as pd

from core.inputs import SparseFeatP
from core.static_dataset import StaticDataset
from core.util import compute_exposure_effect_kuaishouRec, negative_sampling
from deepctr_torch.inputs import DenseFeat

DATAPATH = "environments/KuaishouRec/data"
USER_COLS = ["user_id"]
ITEM_COLS = ["photo_id", "feat0", "feat1", "feat2", "feat3", "photo_duration"]


def item_feature_table(datapath):
    """(list_feat, df_feat): category lists per photo id and the 4-column table shifted by one (0 = padding)."""
    with open(os.path.join(datapath, "item_categories.json")) as fh:
        raw = json.load(fh)
    list_feat = [raw[str(i)]["feature_index"] for i in range(len(raw))]
    df_feat = pd.DataFrame(list_feat, columns=["feat0", "feat1", "feat2", "feat3"])
    df_feat.index.name = "photo_id"
    df_feat = (df_feat.fillna(-1) + 1).astype(int)
    return list_feat, df_feat


def feature_columns(n_user, n_photo, n_feat, entity_dim, feature_dim):
    """The 7 input columns of the DeepFM user model: user, photo, four category slots sharing one table (0 = padding), duration."""
    cols = [SparseFeatP("user_id", n_user, embedding_dim=entity_dim), SparseFeatP("photo_id", n_photo, embedding_dim=entity_dim)]
    cols += [SparseFeatP(f"feat{i}", n_feat, embedding_dim=feature_dim, embedding_name="feat", padding_idx=0) for i in range(4)]
    return cols + [DenseFeat("photo_duration", 1)]


def load_static_validate_data_kuaishou(entity_dim, feature_dim, datapath=None):
    """Validation set = the fully observed small matrix (reference core/util.py:81-133) + the evaluation env's item table."""
    datapath = DATAPATH if datapath is None else datapath
    small = pd.read_csv(os.path.join(datapath, "small_matrix.csv"), usecols=["user_id", "photo_id", "watch_ratio", "photo_duration"])
    small["photo_duration"] /= 1000
    _, df_feat = item_feature_table(datapath)
    small = small.join(df_feat, on=["photo_id"], how="left")
    small.loc[small["watch_ratio"] > 5, "watch_ratio"] = 5
    x_columns = feature_columns(small["user_id"].max() + 1, small["photo_id"].max() + 1, df_feat.max().max() + 1, entity_dim, feature_dim)
    with open(os.path.join(datapath, "photo_mean_duration.json")) as fh:
        mean_dur = {int(k): v for k, v in json.load(fh).items()}
    dataset_val = StaticDataset(x_columns, [DenseFeat("y", 1)], num_workers=4)
    dataset_val.compile_dataset(small[USER_COLS + ITEM_COLS], small[["watch_ratio"]])
    dataset_val.set_env_items(small, df_feat, mean_dur)
    return dataset_val


def _big_log(datapath):
    """big_matrix.csv joined with the item categories, durations in seconds, the watch ratio clipped at 5 -> (big, list_feat, df_feat)."""
    big = pd.read_csv(os.path.join(datapath, "big_matrix.csv"), usecols=["user_id", "photo_id", "timestamp", "watch_ratio", "photo_duration"])
    big["photo_duration"] /= 1000
    list_feat, df_feat = item_feature_table(datapath)
    big = big.join(df_feat, on=["photo_id"], how="left")
    big.loc[big["watch_ratio"] > 5, "watch_ratio"] = 5
    return big, list_feat, df_feat


def load_log_kuaishou(datapath=None):
    """The training log as the LinUCB baseline reads it (core/policy/linucb.py: linucb_trainer's df_x, df_y): the seven columns
    [user_id, photo_id, feat0..3, photo_duration] of every row of big_matrix.csv and its watch ratio; no negatives, no exposure."""
    big, _, _ = _big_log(DATAPATH if datapath is None else datapath)
    return big[USER_COLS + ITEM_COLS], big[["watch_ratio"]]


def _training_log(entity_dim, feature_dim, datapath):
    """The part the three training-set loaders share: big_matrix.csv joined with the item categories, the feature columns, and the
    positive pair columns next to one sampled negative per row.  -> (big, list_feat, x_columns, y_columns, pos_x, pos_y, x_all)"""
    big, list_feat, df_feat = _big_log(datapath)
    x_columns = feature_columns(big["user_id"].max() + 1, big["photo_id"].max() + 1, df_feat.max().max() + 1, entity_dim, feature_dim)
    y_columns = [DenseFeat("y", 1)]
    pos_x, pos_y = big[USER_COLS + ITEM_COLS], big[["watch_ratio"]]
    neg = negative_sampling(big, df_feat, datapath)
    neg_x = neg[USER_COLS + ITEM_COLS].rename(columns=lambda c: c + "_neg")
    return big, list_feat, x_columns, y_columns, pos_x, pos_y, pd.concat([pos_x, neg_x], axis=1)


def load_dataset_kuaishou(tau, entity_dim, feature_dim, MODEL_SAVE_PATH, datapath=None):
    """-> (StaticDataset, x_columns, y_columns, ab_columns) exactly as the reference assembles them."""
    datapath = DATAPATH if datapath is None else datapath
    big, list_feat, x_columns, y_columns, pos_x, pos_y, x_all = _training_log(entity_dim, feature_dim, datapath)
    n_user, n_photo = big["user_id"].max() + 1, big["photo_id"].max() + 1
    ab_columns = [SparseFeatP("alpha_u", n_user, embedding_dim=1), SparseFeatP("beta_i", n_photo, embedding_dim=1)]

    if tau == 0:
        exposure = np.zeros([len(x_all), 1])
    else:
        exposure = compute_exposure_effect_kuaishouRec(pos_x, big["timestamp"], list_feat, tau, MODEL_SAVE_PATH, datapath)

    dataset = StaticDataset(x_columns, y_columns, num_workers=4)
    dataset.compile_dataset(x_all, pos_y, exposure)
    return dataset, x_columns, y_columns, ab_columns


def load_dataset_kuaishou_IPS_pairwise(entity_dim, feature_dim, datapath=None):
    """The training set of DeepFM-IPS-pairwise.py:89-146: the score column is the inverse propensity of the row's item,
    1 / (its number of rows in the log) (compute_IPS_kuaishouRec, :79-86), counted on the device.  -> (StaticDataset, x_columns, y_columns)"""
    from cirs_hip.dataprep import ips_scores
    datapath = DATAPATH if datapath is None else datapath
    big, _, x_columns, y_columns, _, pos_y, x_all = _training_log(entity_dim, feature_dim, datapath)
    dataset = StaticDataset(x_columns, y_columns, num_workers=4)
    dataset.compile_dataset(x_all, pos_y, ips_scores(big["photo_id"].to_numpy()))
    return dataset, x_columns, y_columns


def load_dataset_kuaishou_PD(entity_dim, feature_dim, gamma, datapath=None):
    """The training set of PD-pairwise.py:111-168: the score column is (the share of the row's item among the log rows of the row's
    time bin) ** gamma (compute_popularity_kuaishouRec_pairwise, :76-108; five bins), counted on the device.  The reference reads
    `args.gamma` from a module global; here it is a parameter.  -> (StaticDataset, x_columns, y_columns)"""
    from cirs_hip.dataprep import popularity_scores
    datapath = DATAPATH if datapath is None else datapath
    big, _, x_columns, y_columns, _, pos_y, x_all = _training_log(entity_dim, feature_dim, datapath)
    dataset = StaticDataset(x_columns, y_columns, num_workers=4)
    dataset.compile_dataset(x_all, pos_y, popularity_scores(big["photo_id"].to_numpy(), big["timestamp"].to_numpy(), gamma))
    return dataset, x_columns, y_columns


def dice_feature_columns(n_user, n_photo, n_feat, entity_dim, feature_dim):
    """The 16 input columns of the DICE model (DICE.py:119-144): interest and conformity copies of the user and the photo id, four
    category slots sharing one table (0 = padding), duration; then the negative item's photo copies, slots and duration."""
    def item(sfx):
        return [SparseFeatP("photo_id_int" + sfx, n_photo, embedding_dim=entity_dim, embedding_name="photo_int"),
                SparseFeatP("photo_id_con" + sfx, n_photo, embedding_dim=entity_dim, embedding_name="photo_con")] + \
               [SparseFeatP(f"feat{i}{sfx}", n_feat, embedding_dim=feature_dim, embedding_name="feat", padding_idx=0) for i in range(4)] + \
               [DenseFeat("photo_duration" + sfx, 1)]
    return [SparseFeatP("user_id_int", n_user, embedding_dim=entity_dim, embedding_name="user_int"),
            SparseFeatP("user_id_con", n_user, embedding_dim=entity_dim, embedding_name="user_con")] + item("") + item("_neg")


def dice_conformity_score(photo_pos, photo_neg, photo_log):
    """compute_popularity_kuaishouRec and the sign rule of DICE.py:77-87, 175-177: an item's popularity is its number of rows in the whole
    log (an item the log does not hold counts 1); +1 where the positive is the more popular item, -1 otherwise (ties included).
    -> int64 [n, 1]"""
    photo_pos, photo_neg, photo_log = (np.asarray(a, np.int64).reshape(-1) for a in (photo_pos, photo_neg, photo_log))
    count = np.bincount(photo_log, minlength=int(max(photo_pos.max(), photo_neg.max())) + 1)
    pop_pos, pop_neg = np.maximum(count[photo_pos], 1), np.maximum(count[photo_neg], 1)
    return np.where(pop_pos > pop_neg, 1, -1).astype(np.int64)[:, None]


def load_dataset_kuaishou_DICE(entity_dim, feature_dim, datapath=None):
    """The training set of DICE.py:90-182: the user and the photo id of the positive row in an interest and a conformity column each, the
    sampled negative's photo id likewise, and the conformity score of the pair as the score column.
    -> (StaticDataset, x_columns, y_columns)"""
    datapath = DATAPATH if datapath is None else datapath
    big, _, _, y_columns, pos_x, pos_y, x_all = _training_log(entity_dim, feature_dim, datapath)
    _, df_feat = item_feature_table(datapath)
    x_columns = dice_feature_columns(big["user_id"].max() + 1, big["photo_id"].max() + 1, df_feat.max().max() + 1, entity_dim, feature_dim)
    item = ["feat0", "feat1", "feat2", "feat3", "photo_duration"]
    x16 = pd.concat([x_all[["user_id", "user_id", "photo_id", "photo_id"] + item],
                     x_all[["photo_id_neg", "photo_id_neg"] + [c + "_neg" for c in item]]], axis=1)
    x16.columns = [c.name for c in x_columns]
    score = dice_conformity_score(pos_x["photo_id"].to_numpy(), x_all["photo_id_neg"].to_numpy(), big["photo_id"].to_numpy())
    dataset = StaticDataset(x_columns, y_columns, num_workers=4)
    dataset.compile_dataset(x16, pos_y, score)
    return dataset, x_columns, y_columns
