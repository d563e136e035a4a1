"""The disjoint-arm LinUCB baseline (reference core/policy/linucb.py) over the device state of cirs_hip.linucb.DeviceLinUCB.

The names and call shapes are the reference's: linucb_policy(K_arms, d, alpha) with select_arm / forward / evaluate_data /
recommend_k_item, its `linucb_arms` views, and linucb_trainer.  What differs is where the work is done:

  linucb_trainer    the reference makes one Python iteration per log row (a LabelEncoder.transform call and a rank-1 update); here the
                    log is uploaded once, grouped by arm once, and every epoch is one ordered accumulation launch whose A and b equal
                    the reference's bit for bit (csrc/linucb.hip).
  recommend_k_item  the reference inverts every arm's A twice per arm and call (theta and A_inv are properties); here the solve runs once
                    after an update and one launch scores every arm and takes the arg-max.
  test_kuaishou     (evaluation.py) one scoring launch for all trajectory users, then one lock-step rollout.

recommend_k_item accepts the epsilon= and is_ucb= that evaluation.test_kuaishou passes (the reference's does not, so its trainer stops
with TypeError after its first epoch); any value but the defaults is refused: LinUCB's exploration is its own bound.
linucb_trainer returns the list of per-epoch result dicts (the reference returns nothing)."""
import numpy as np
import torch

from cirs_hip.linucb import DeviceLinUCB, arm_of_rows
from cirs_hip.linucb_host import tie_pick
from evaluation import test_kuaishou


class linucb_disjoint_arm():
    """A view of one arm of the device state, with the reference's attributes and shapes."""

    def __init__(self, policy, arm_index, alpha):
        self._policy = policy
        self.arm_index = arm_index
        self.alpha = alpha

    @property
    def _state(self):
        return self._policy.device_state

    @property
    def A(self):
        return self._state.A[self.arm_index].cpu().numpy()

    @property
    def b(self):
        return self._state.b[self.arm_index].cpu().numpy().reshape(-1, 1)

    @property
    def A_inv(self):
        return self._state.A_inv[self.arm_index].cpu().numpy()

    @property
    def theta(self):
        return self._state.theta[self.arm_index].cpu().numpy().reshape(-1, 1)

    def calc_reward(self, x_array):
        _, mean = self._state.score_x(np.asarray(x_array, np.float64).reshape(-1))
        return mean[self.arm_index].cpu().numpy().reshape(1, 1)

    def calc_UCB(self, x_array):
        ucb, _ = self._state.score_x(np.asarray(x_array, np.float64).reshape(-1))
        return ucb[self.arm_index].cpu().numpy().reshape(1, 1)

    def reward_update(self, reward, x_array):
        self._state.update_one(self.arm_index, reward, np.asarray(x_array, np.float64).reshape(-1))


class linucb_policy():

    def __init__(self, K_arms, d, alpha, device="cuda"):
        self.K_arms = K_arms
        self._shape = (K_arms, d, alpha, device)
        self._state = None
        self.linucb_arms = [linucb_disjoint_arm(self, arm_index=i, alpha=alpha) for i in range(K_arms)]
        self._classes = None

    @property
    def device_state(self):
        """The arms' A, b, inv(A), theta on the device (cirs_hip.linucb.DeviceLinUCB), allocated at first use."""
        if self._state is None:
            K, d, alpha, device = self._shape
            self._state = DeviceLinUCB(K, d, alpha, device=device)
        return self._state

    def _arm_of_rows(self, x, lbe_photo):
        """Arm of every row of the device tensor x [n, d]: the position of int(x[1]) in lbe_photo.classes_, -1 when it is absent."""
        classes = np.asarray(lbe_photo.classes_).astype(np.int64)
        if self._classes is None or not np.array_equal(self._classes[0], classes):
            assert np.all(classes[1:] > classes[:-1]), "lbe_photo.classes_ must be sorted (LabelEncoder's are)"
            self._classes = (classes, torch.as_tensor(classes).to(self.device_state.device))
        return arm_of_rows(self._classes[1], x[:, 1].to(torch.int64))

    def select_arm(self, x_array):
        ucb, _ = self.device_state.score_x(np.asarray(x_array, np.float64).reshape(-1))
        return tie_pick(ucb.cpu().numpy())

    def forward(self, arm, x_array):
        return self.linucb_arms[arm].calc_reward(x_array)

    def evaluate_data(self, dataset_val, metric_fun, lbe_photo):
        y = dataset_val.get_y()
        x_val = torch.as_tensor(np.ascontiguousarray(dataset_val.x_numpy, dtype=np.float64)).to(self.device_state.device)
        pred = self.device_state.predict(x_val, self._arm_of_rows(x_val, lbe_photo))
        y_predict = np.zeros_like(y)
        y_predict[...] = pred.cpu().numpy().reshape(y_predict.shape)
        eval_result = {}
        for name, fun in metric_fun.items():
            eval_result[name] = fun(y, y_predict)
        return eval_result

    def recommend_k_item(self, user, dataset_val, k=1, is_softmax=True, epsilon=0, is_ucb=False):  # for kuaishou data
        if epsilon != 0 or is_ucb:
            raise ValueError("linucb_policy.recommend_k_item explores through its own upper confidence bound: epsilon must be 0 and "
                             "is_ucb False")
        df_photo_env = dataset_val.df_photo_env
        best, mean = self.device_state.score(np.asarray([user], np.float64), df_photo_env.to_numpy())
        index = int(best[0])
        recommendation = df_photo_env.index.to_numpy()[index]
        return recommendation, float(mean[0])


def linucb_trainer(model, env, epoch, df_x, df_y, dataset_val, logger, metric_fun):
    state = model.device_state
    x = torch.as_tensor(np.ascontiguousarray(df_x.to_numpy(), dtype=np.float64)).to(state.device)      # the log goes up once
    y = torch.as_tensor(np.ascontiguousarray(df_y.to_numpy(), dtype=np.float64).reshape(-1)).to(state.device)
    plan = state.plan(model._arm_of_rows(x, env.lbe_photo))
    history = []
    for epo in range(epoch):
        state.update(x, y, plan=plan)

        eval_result = model.evaluate_data(dataset_val, metric_fun, env.lbe_photo)
        eval_result_RL = test_kuaishou(model, env=env, dataset_val=dataset_val, is_softmax=False)

        eval_result = {"val_" + k: v for k, v in eval_result.items()}
        eval_result_RL = {"RL_val_" + k: v for k, v in eval_result_RL.items()}
        result = {}
        result.update(eval_result)
        result.update(eval_result_RL)

        logger.info("Epoch: [{}], Info: [{}]".format(epo, result))
        history.append(result)
    return history
