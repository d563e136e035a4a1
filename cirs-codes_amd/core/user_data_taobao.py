"""The VirtualTaobao user-model training set (reference CIRS-UserModel-taobao.py:52-112, `load_dataset_virtualTaobao`): a
`dataset.txt`-shaped log -- per line the 91-column state (88 user features, the two last-action columns, the turn counter), the
27-column action and the clicks, separated by spaces or commas -- and the exposure effect of every row, computed on the device
(cirs_vtb_exposure_history)."""
import re

import numpy as np
import pandas as pd

from core.static_dataset import StaticDataset
from deepctr_torch.inputs import DenseFeat

FILENAME = "environments/VirtualTaobao/virtualTB/SupervisedLearning/dataset.txt"
USER_FEATURES = ["feat" + str(i) for i in range(91)]
ITEM_FEATURES = ["y" + str(i) for i in range(27)]
REWARD_FEATURES = ["click"]


def read_log(filename):
    """-> DataFrame with the columns feat0..feat90, y0..y26, click."""
    cols = USER_FEATURES + ITEM_FEATURES + REWARD_FEATURES
    rows = []
    with open(filename) as fh:
        for ln, line in enumerate(fh):
            parts = [p for p in re.split(r"[\s,]+", line.strip()) if p]
            if not parts:
                continue
            if len(parts) != len(cols):
                raise ValueError(f"{filename}:{ln + 1}: {len(parts)} columns, expected {len(cols)}")
            rows.append(parts)
    return pd.DataFrame(np.asarray(rows, dtype=np.float64).reshape(-1, len(cols)), columns=cols)


def compute_exposure_effect_virtualTaobao(df_x, tau, device="cuda"):
    """[n, 1] float64: for every row the sum over the earlier rows j of its session of exp(-(r - j) * ||a_r - a_j||_2 / tau); the turn
    column feat90 == 1 opens a session."""
    from cirs_hip.mmoe_train import vtb_exposure_history
    timestamp = df_x["feat90"].to_numpy().astype(int)
    action = df_x[ITEM_FEATURES].to_numpy()
    return vtb_exposure_history(timestamp, action, tau, device=device).cpu().numpy()


def load_dataset_virtualTaobao(tau, filename=FILENAME, feature_dim=10, exposure_fn=None):
    """-> (StaticDataset, x_columns, y_columns) like the reference.  exposure_fn(df_x, tau) replaces the device computation (tests)."""
    df = read_log(filename)
    df_x, df_y = df[USER_FEATURES + ITEM_FEATURES], df[REWARD_FEATURES]
    x_columns = [DenseFeat("user_feat", 91)] + [DenseFeat("feat_item", 27)]      # no exposure column among the features
    y_columns = [DenseFeat("y", 1)]
    exposure_all = (exposure_fn or compute_exposure_effect_virtualTaobao)(df_x, tau)
    dataset = StaticDataset(x_columns, y_columns, num_workers=4)
    dataset.compile_dataset(df_x, df_y, exposure_all)
    return dataset, x_columns, y_columns


def load_dataset_mlp_taobao(filename=FILENAME, feature_dim=10):
    """`load_dataset_virtualTaobao` of the static baselines (reference MLP-taobao.py:51-71, the same lines in
    MLP-epsilonGreedy-taobao.py) over the same 91 + 27 + 1 column log: x = the 91-column static state, y = [27 item features | click];
    there is no exposure column.  -> (StaticDataset with x_numpy [n, 91] and y_numpy [n, 28], x_columns, y_columns)."""
    df = read_log(filename)
    df_x, df_y = df[USER_FEATURES], df[ITEM_FEATURES + REWARD_FEATURES]
    x_columns = [DenseFeat("feat_user", 91)]
    y_columns = [DenseFeat("feat_item", 27)] + [DenseFeat("y", 1)]
    dataset = StaticDataset(x_columns, y_columns, num_workers=4)
    dataset.compile_dataset(df_x, df_y)
    return dataset, x_columns, y_columns
