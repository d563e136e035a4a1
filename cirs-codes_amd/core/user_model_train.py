"""The user-model training run of the reference (CIRS-UserModel-kuaishou.py:152-255, `main`) as one function: KuaiRec files ->
training / validation sets (core.user_data) -> UserModel_Pairwise fitted on the device -> the three artefacts the RL script
loads (`<name>_params_<msg>.pickle`, `normed_mat-<msg>.pickle`, `<name>_<msg>.pt`).  Logging, argument parsing and the upload
hook of the script are not part of it."""
import os
import pickle
from types import SimpleNamespace

import torch

from core.user_data import load_dataset_kuaishou, load_static_validate_data_kuaishou
from core.user_model_pairwise import UserModel_Pairwise, make_loss_kuaishou_pairwise
from environments.KuaishouRec.env.kuaishouEnv import KuaishouEnv

DEFAULTS = dict(env="KuaishouEnv-v0", user_model_name="DeepFM", message="UM", tau=1000.0, feature_dim=8, dnn=(64, 64),
                l2_reg_dnn=0.1, lambda_ab=10.0, is_ab=True, batch_size=2048, epoch=5, lr=1e-3, seed=2022)


class _RLTest:   # epoch-end hook in the position of compile_RL_test
    def __init__(self, model, rl_test):
        self.model, self.rl_test = model, rl_test

    def on_train_begin(self): pass
    def on_train_end(self): pass
    def on_epoch_begin(self, epoch): pass

    def on_epoch_end(self, epoch, logs):
        if self.rl_test is not None:
            logs["RL_val"] = self.rl_test(self.model, epoch)


class EpochLines:
    """Callback that keeps (epoch, logs) of every on_epoch_end call, epoch -1 (the untrained model) included, and prints one line per
    call in the manner of the scripts' LoggerCallback_Update."""
    def __init__(self, echo=True):
        self.records, self.echo = [], echo

    def on_train_begin(self): pass
    def on_train_end(self): pass
    def on_epoch_begin(self, epoch): pass

    def on_epoch_end(self, epoch, logs):
        self.records.append((epoch, dict(logs)))
        if self.echo:
            print("Epoch: [{}], Info: [{}]".format(epoch, logs), flush=True)


def _write_artefacts(model, params, a, model_dir, lbe_user, lbe_photo, val_set):
    """The three files the RL script loads: constructor parameters, the normalised reward table, the state dict (on the CPU)."""
    paths = SimpleNamespace(params=os.path.join(model_dir, "{}_params_{}.pickle".format(a.user_model_name, a.message)),
                            normed_mat=os.path.join(model_dir, "normed_mat-{}.pickle".format(a.message)),
                            state_dict=os.path.join(model_dir, "{}_{}.pt".format(a.user_model_name, a.message)))
    with open(paths.params, "wb") as fh:
        pickle.dump(dict(params, device="cpu"), fh)
    normed_mat = KuaishouEnv.compute_normed_reward(model, lbe_user, lbe_photo, val_set.df_photo_env)
    with open(paths.normed_mat, "wb") as fh:
        pickle.dump(normed_mat, fh)
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, paths.state_dict)
    return paths, normed_mat


def train_user_model(datapath, save_root=".", callbacks=None, rl_test=None, metric_fun=None, **overrides):
    """Returns SimpleNamespace(model, history, normed_mat, paths).  rl_test(model, epoch) (optional) is called after every epoch,
    the place of the reference's compile_RL_test hook (e.g. a partial of evaluation.test_static_model_in_RL_env); a hook of the
    reference's own shape, fn(model) -> dict, goes through `model.compile_RL_test` by the caller instead.  metric_fun: the script's
    {"mae": ..., "mse": ...} (core.user_model.metric_mae / metric_mse run fused on the device): evaluated on the validation set before
    training (epoch -1 of the callbacks) and after every epoch, into the epoch's logs; None keeps the logs at {"loss"}."""
    a = SimpleNamespace(**{**DEFAULTS, **overrides})
    entity_dim = a.feature_dim
    model_dir = os.path.join(save_root, "saved_models", a.env, a.user_model_name)
    os.makedirs(os.path.join(model_dir, "logs"), exist_ok=True)

    mat, lbe_user, lbe_photo, list_feat, df_photo_env, df_dist_small = KuaishouEnv.load_mat(datapath)
    train_set, x_columns, y_columns, ab_columns = load_dataset_kuaishou(a.tau, entity_dim, a.feature_dim, model_dir, datapath=datapath)
    if not a.is_ab:
        ab_columns = None
    val_set = load_static_validate_data_kuaishou(entity_dim, a.feature_dim, datapath)

    params = {"feature_columns": x_columns, "y_columns": y_columns, "task": "regression", "task_logit_dim": 1,
              "dnn_hidden_units": tuple(a.dnn), "seed": a.seed, "device": "cuda", "ab_columns": ab_columns}
    model = UserModel_Pairwise(l2_reg_dnn=a.l2_reg_dnn, **params)
    model.compile(torch.optim.Adam(model.parameters(), lr=a.lr), loss_func=make_loss_kuaishou_pairwise(a.lambda_ab), metric_fun=metric_fun)

    history = model.fit_data(train_set, val_set, batch_size=a.batch_size, epochs=a.epoch, callbacks=list(callbacks or []) + [_RLTest(model, rl_test)])

    paths, normed_mat = _write_artefacts(model, params, a, model_dir, lbe_user, lbe_photo, val_set)
    return SimpleNamespace(model=model, history=history, normed_mat=normed_mat, paths=paths, val_set=val_set,
                           lbe_user=lbe_user, lbe_photo=lbe_photo)


DEBIAS_DEFAULTS = dict(env="KuaishouEnv-v0", feature_dim=16, dnn=(64, 64), l2_reg_dnn=0.1, batch_size=2048, epoch=50, lr=1e-3, seed=2021,
                       gamma=0.1)
DEBIAS_NAMES = {"ips": "DeepFM-IPS-pairwise", "pd": "PD-pairwise"}


def train_debias_kuaishou(datapath, method="ips", save_root=".", callbacks=None, rl_test=None, metric_fun=None, **overrides):
    """The training runs of the two debiasing baselines (DeepFM-IPS-pairwise.py:149-239, PD-pairwise.py:171-238, `main`): KuaiRec files
    -> training set with the method's score column (core.user_data) -> UserModel_Pairwise without alpha/beta fitted on the device with
    the method's loss.  rl_test(model, epoch) sits where the scripts' compile_RL_test hook sits, metric_fun as in train_user_model.  "ips" writes the three artefacts its
    script writes (`<name>_params_<msg>.pickle`, `normed_mat-<msg>.pickle`, `<name>_<msg>.pt`); "pd", like its script, writes none.
    Returns SimpleNamespace(model, history, normed_mat, paths, val_set, lbe_user, lbe_photo), normed_mat and paths None for "pd"."""
    from core.user_data import load_dataset_kuaishou_IPS_pairwise, load_dataset_kuaishou_PD
    from core.user_model_pairwise import loss_kuaishou_IPS_pairwise, loss_kuaishou_PD_pairwise
    if method not in DEBIAS_NAMES:
        raise ValueError(f"method must be 'ips' or 'pd', got {method!r}")
    name = DEBIAS_NAMES[method]
    a = SimpleNamespace(**{**DEBIAS_DEFAULTS, "user_model_name": name, "message": name, **overrides})
    entity_dim = a.feature_dim
    model_dir = os.path.join(save_root, "saved_models", a.env, a.user_model_name)
    os.makedirs(os.path.join(model_dir, "logs"), exist_ok=True)

    mat, lbe_user, lbe_photo, list_feat, df_photo_env, df_dist_small = KuaishouEnv.load_mat(datapath)
    if method == "ips":
        train_set, x_columns, y_columns = load_dataset_kuaishou_IPS_pairwise(entity_dim, a.feature_dim, datapath=datapath)
    else:
        train_set, x_columns, y_columns = load_dataset_kuaishou_PD(entity_dim, a.feature_dim, a.gamma, datapath=datapath)
    val_set = load_static_validate_data_kuaishou(entity_dim, a.feature_dim, datapath)

    params = {"feature_columns": x_columns, "y_columns": y_columns, "task": "regression", "task_logit_dim": 1,
              "dnn_hidden_units": tuple(a.dnn), "seed": a.seed, "device": "cuda"}
    model = UserModel_Pairwise(l2_reg_dnn=a.l2_reg_dnn, **params)
    model.compile(torch.optim.Adam(model.parameters(), lr=a.lr),
                  loss_func=loss_kuaishou_IPS_pairwise if method == "ips" else loss_kuaishou_PD_pairwise, metric_fun=metric_fun)

    history = model.fit_data(train_set, val_set, batch_size=a.batch_size, epochs=a.epoch, callbacks=list(callbacks or []) + [_RLTest(model, rl_test)])
    paths, normed_mat = _write_artefacts(model, params, a, model_dir, lbe_user, lbe_photo, val_set) if method == "ips" else (None, None)
    return SimpleNamespace(model=model, history=history, normed_mat=normed_mat, paths=paths, val_set=val_set,
                           lbe_user=lbe_user, lbe_photo=lbe_photo)


DICE_DEFAULTS = dict(env="KuaishouEnv-v0", user_model_name="DICE", message="DICE", feature_dim=16, dnn=(64, 64), l2_reg_dnn=0.1, batch_size=2048,
                     epoch=50, lr=1e-3, seed=2021)


def train_dice_kuaishou(datapath, save_root=".", callbacks=None, rl_test=None, metric_fun=None, **overrides):
    """The training run of the DICE baseline (DICE.py:185-261, `main`): KuaiRec files -> the 16-column training set with the conformity
    score (core.user_data.load_dataset_kuaishou_DICE) -> UserModel_DICE fitted on the device with loss_kuaishou_DICE.  rl_test(model) ->
    dict goes through compile_RL_test, like the script's partial of test_static_model_in_RL_env: it is called on the untrained model
    (epoch -1) and after every epoch, its results joining the epoch's logs, behind the validation metrics of metric_fun (as in
    train_user_model).  Like the script, the run writes one artefact, the
    constructor parameters (`<name>_params_<msg>.pickle`).
    Returns SimpleNamespace(model, history, paths, train_set, val_set, lbe_user, lbe_photo)."""
    from core.user_data import load_dataset_kuaishou_DICE
    from core.user_model_DICE import UserModel_DICE, loss_kuaishou_DICE
    a = SimpleNamespace(**{**DICE_DEFAULTS, **overrides})
    entity_dim = a.feature_dim
    model_dir = os.path.join(save_root, "saved_models", a.env, a.user_model_name)
    os.makedirs(os.path.join(model_dir, "logs"), exist_ok=True)

    mat, lbe_user, lbe_photo, list_feat, df_photo_env, df_dist_small = KuaishouEnv.load_mat(datapath)
    train_set, x_columns, y_columns = load_dataset_kuaishou_DICE(entity_dim, a.feature_dim, datapath=datapath)
    val_set = load_static_validate_data_kuaishou(entity_dim, a.feature_dim, datapath)

    params = {"feature_columns": x_columns, "y_columns": y_columns, "task": "regression", "task_logit_dim": 1,
              "dnn_hidden_units": tuple(a.dnn), "seed": a.seed, "device": "cuda"}
    model = UserModel_DICE(l2_reg_dnn=a.l2_reg_dnn, **params)
    model.compile(torch.optim.Adam(model.parameters(), lr=a.lr), loss_func=loss_kuaishou_DICE, metric_fun=metric_fun)
    if rl_test is not None:
        model.compile_RL_test(rl_test)

    history = model.fit_data(train_set, val_set, batch_size=a.batch_size, epochs=a.epoch, callbacks=list(callbacks or []))
    paths = SimpleNamespace(params=os.path.join(model_dir, "{}_params_{}.pickle".format(a.user_model_name, a.message)))
    with open(paths.params, "wb") as fh:
        pickle.dump(dict(params, device="cpu"), fh)
    return SimpleNamespace(model=model, history=history, paths=paths, train_set=train_set, val_set=val_set, lbe_user=lbe_user, lbe_photo=lbe_photo)


LINUCB_DEFAULTS = dict(env="KuaishouEnv-v0", model_name="LinUCB", message="LinUCB", alpha=0.25, epoch=5, feature_dim=8, num_leave_compute=1,
                       leave_threshold=0, max_turn=100)


def train_linucb_kuaishou(datapath, save_root=".", logger=None, metric_fun=None, **overrides):
    """The run of the LinUCB baseline (core/policy/linucb.py; the reference ships the module without a script, so the steps are those of
    the other Kuaishou baselines): KuaiRec files -> the training log as df_x (the seven columns [user, photo, feat0..3, duration]) and
    df_y (the watch ratio), the validation set and the evaluation env -> linucb_policy with one arm per env item, d = 2 + the width of
    df_photo_env -> linucb_trainer on the device: per epoch one ordered accumulation over the log, the validation metrics of
    metric_fun (default: the scripts' mae and mse) and evaluation.test_kuaishou, one log line each.  `logger`: anything with
    .info(str); default: lines are kept only in the returned history.
    Returns SimpleNamespace(model, history, val_set, lbe_user, lbe_photo), history = linucb_trainer's per-epoch result dicts."""
    from core.policy.linucb import linucb_policy, linucb_trainer
    from core.user_data import load_log_kuaishou
    from core.user_model import metric_mae, metric_mse
    a = SimpleNamespace(**{**LINUCB_DEFAULTS, **overrides})
    model_dir = os.path.join(save_root, "saved_models", a.env, a.model_name)
    os.makedirs(os.path.join(model_dir, "logs"), exist_ok=True)

    mat, lbe_user, lbe_photo, list_feat, df_photo_env, df_dist_small = KuaishouEnv.load_mat(datapath)
    df_x, df_y = load_log_kuaishou(datapath)
    val_set = load_static_validate_data_kuaishou(a.feature_dim, a.feature_dim, datapath)
    env = KuaishouEnv(mat, lbe_user, lbe_photo, list_feat, df_photo_env, df_dist_small, num_leave_compute=a.num_leave_compute,
                      leave_threshold=a.leave_threshold, max_turn=a.max_turn)

    model = linucb_policy(len(val_set.df_photo_env), 2 + val_set.df_photo_env.shape[1], a.alpha)
    if logger is None:
        logger = SimpleNamespace(info=lambda msg: None)
    if metric_fun is None:
        metric_fun = {"mae": metric_mae, "mse": metric_mse}
    history = linucb_trainer(model, env, a.epoch, df_x, df_y, val_set, logger, metric_fun)
    return SimpleNamespace(model=model, history=history, val_set=val_set, lbe_user=lbe_user, lbe_photo=lbe_photo)


TAOBAO_DEFAULTS = dict(env="VirtualTB-v0", user_model_name="MLP", message="UM", tau=0.01, feature_dim=8, dnn=(64, 64), batch_size=100,
                       epoch=5, seed=2022)


def train_user_model_taobao(dataset_path, save_root=".", callbacks=None, exposure_fn=None, shuffle=True, **overrides):
    """The user-model training run of CIRS-UserModel-taobao.py:115-182 (`main`) without logging: the `dataset.txt`-shaped log ->
    training set with its exposure effect -> UserModel_MMOE fitted on the device -> the two artefacts CIRS-RL-taobao.py:134-142 loads
    (`<name>_params_<msg>.pickle`, `<name>_<msg>.pt`) under saved_models/VirtualTB-v0/<name>/, weights saved on the CPU.
    Returns SimpleNamespace(model, history, paths, dataset).  The device SimulatedEnv steps a (128, 128) model only: pass
    dnn=(128, 128) when the trained model is to drive `SimulatedEnv.build_device_env` (the script's default is (64, 64))."""
    import collections
    from core.user_data_taobao import load_dataset_virtualTaobao
    from core.user_model_mmoe import UserModel_MMOE, loss_taobao
    from deepctr_torch.inputs import DenseFeat
    a = SimpleNamespace(**{**TAOBAO_DEFAULTS, **overrides})
    model_dir = os.path.join(save_root, "saved_models", a.env, a.user_model_name)
    os.makedirs(os.path.join(model_dir, "logs"), exist_ok=True)
    dataset, x_columns, y_columns = load_dataset_virtualTaobao(a.tau, dataset_path, feature_dim=a.feature_dim, exposure_fn=exposure_fn)
    tasks = collections.OrderedDict({feat.name: "regression" for feat in y_columns})
    task_logit_dim = {feat.name: feat.dimension if isinstance(feat, DenseFeat) else feat.embedding_dim for feat in y_columns}
    params = {"feature_columns": x_columns, "y_columns": y_columns, "num_tasks": len(tasks), "tasks": tasks, "task_logit_dim": task_logit_dim,
              "dnn_hidden_units": tuple(a.dnn), "seed": a.seed, "device": "cpu"}
    model = UserModel_MMOE(**params)
    model.compile(optimizer="adam", loss_func=loss_taobao, metrics=None)
    history = model.fit_data(dataset, batch_size=a.batch_size, epochs=a.epoch, callbacks=list(callbacks or []), shuffle=shuffle) if a.epoch > 0 else []
    paths = SimpleNamespace(params=os.path.join(model_dir, "{}_params_{}.pickle".format(a.user_model_name, a.message)),
                            state_dict=os.path.join(model_dir, "{}_{}.pt".format(a.user_model_name, a.message)))
    with open(paths.params, "wb") as fh:
        pickle.dump(params, fh)
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, paths.state_dict)
    return SimpleNamespace(model=model, history=history, paths=paths, dataset=dataset)


MLP_TAOBAO_DEFAULTS = dict(env="VirtualTB-v0", model_name="MLP", message="MLP", feature_dim=4, dnn=(256, 256), batch_size=100, epoch=100,
                           leave_threshold=1.0, num_leave_compute=5, max_turn=50, seed=2022, num_trajectory=100)


def train_mlp_taobao(dataset_path, save_root=".", callbacks=None, epsilon=0, shuffle=True, vtb_env=None, **overrides):
    """The static baselines' run (MLP-taobao.py:74-132, `main`; epsilon > 0: MLP-epsilonGreedy-taobao.py) step for step, training and
    the per-epoch evaluation on the device: create the directories, a VirtualTB in static-state mode, the 91 + 27 + 1 column log ->
    data set, the two-task UserModel_MMOE, compile("adam", loss_taobao_mlp), compile_RL_test(test_taobao on the device), fit_data with
    LoggerCallback_Update.  `vtb_env`: a VirtualTB to use instead of a fresh one (it is put into static-state mode).
    Returns SimpleNamespace(model, history, env, dataset, logger_path)."""
    import collections
    import datetime
    import functools
    import time
    from core.user_data_taobao import load_dataset_mlp_taobao
    from core.user_model_mmoe import UserModel_MMOE, loss_taobao_mlp
    from deepctr_torch.inputs import DenseFeat
    from evaluation import test_taobao
    from util.utils import LoggerCallback_Update, create_dir
    a = SimpleNamespace(**{**MLP_TAOBAO_DEFAULTS, **overrides})
    # 1. Create dirs
    model_dir = os.path.join(save_root, "saved_models", a.env, a.model_name)
    create_dir([os.path.join(save_root, "saved_models"), os.path.join(save_root, "saved_models", a.env), model_dir, os.path.join(model_dir, "logs")])
    nowtime = datetime.datetime.fromtimestamp(time.time()).strftime("%Y_%m_%d-%H_%M_%S")
    logger_path = os.path.join(model_dir, "logs", "[{}]_{}.log".format(a.message, nowtime))
    # 2. Prepare Envs
    env = vtb_env
    if env is None:
        from environments.VirtualTaobao.virtualTB.envs.virtualTB import VirtualTB
        env = VirtualTB(num_leave_compute=a.num_leave_compute, leave_threshold=a.leave_threshold, max_turn=a.max_turn)
    env.set_state_mode(True)             # return the states as user initial profile vectors
    # 3. Prepare dataset
    dataset, x_columns, y_columns = load_dataset_mlp_taobao(dataset_path, feature_dim=a.feature_dim)
    # 4. Setup model
    tasks = collections.OrderedDict({feat.name: "regression" for feat in y_columns})
    task_logit_dim = {feat.name: feat.dimension if isinstance(feat, DenseFeat) else feat.embedding_dim for feat in y_columns}
    model = UserModel_MMOE(x_columns, y_columns, len(tasks), tasks, task_logit_dim, dnn_hidden_units=tuple(a.dnn), seed=a.seed, device="cpu")
    model.compile(optimizer="adam", loss_func=loss_taobao_mlp, metrics=None)
    model.compile_RL_test(functools.partial(test_taobao, env=env, epsilon=epsilon, device="cuda", num_trajectory=a.num_trajectory))
    # 5. Learn model
    history = model.fit_data(dataset, batch_size=a.batch_size, epochs=a.epoch, callbacks=list(callbacks or []) + [LoggerCallback_Update(logger_path)],
                             shuffle=shuffle)
    return SimpleNamespace(model=model, history=history, env=env, dataset=dataset, logger_path=logger_path)
