"""The reference's training script (Final_Project/pointnet2/train.py, the same file as scripts/2_train_and_eval_modelnet.py) as
functions: the same names, the same rules (``F.cross_entropy``, gradient norm clipped to 1.0, Adam, a learning rate of
``lr / (epoch + 1)`` stepped per epoch, epochs ``start_epoch + 1 .. epochs``, checkpoints ``{'epoch', 'model_state'}`` that
``objects.predict`` and ``detection.detect`` load).  Nothing runs on import; ``main(argv)`` takes the reference's arguments.

What differs from the reference:
  - the gradients of gather / group / three_interpolate run in a fixed order (``pointnet2_utils.fixed_order_gradients``) unless
    ``fixed_order=False`` is passed, so two runs from the same seed see the same gradient bits from these ops;
  - ``tb_log`` and ``log_f`` may be None (no tensorboard dependency);
  - ``test_one_epoch`` returns the confusion matrix in per cent and the ``classification_report`` text instead of drawing them.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.utils import clip_grad_norm_

from . import pointnet2_utils
from .pointnet2_models import PointNet2ClassificationMSG, PointNet2ClassificationSSG
from .resampled_dataset import KITTIPCDClsDataset_Wrapper


def log_print(info, log_f=None):
    """train.py:46-49."""
    print(info)
    if log_f is not None:
        print(info, file=log_f)


def _scalar(tb_log, name, value, step):
    if tb_log is not None:
        tb_log.add_scalar(name, value, step)


def _to_device(batch):
    pts_input, cls_labels = batch
    return pts_input.cuda(non_blocking=True).float(), cls_labels.cuda(non_blocking=True).long().view(-1)


def train_one_epoch(model, train_loader, optimizer, lr_scheduler, epoch, total_it, tb_log=None, log_f=None, fixed_order=True):
    """train.py:51-83 -> total_it after the epoch.  fixed_order decides the gradient path of every forward in here, whatever
    ``set_fixed_order_gradients`` was set to outside: True the fixed-order kernels, False torch's ``scatter_add_``; the outer setting
    is back in place afterwards."""
    model.train()
    log_print('===============TRAIN EPOCH %d================' % epoch, log_f=log_f)
    for it, batch in enumerate(train_loader):
        optimizer.zero_grad()
        pts_input, cls_labels = _to_device(batch)
        with pointnet2_utils.fixed_order_gradients(fixed_order):
            pred_cls = model(pts_input)
        loss = F.cross_entropy(pred_cls, cls_labels)
        loss.backward()
        clip_grad_norm_(model.parameters(), 1.0)
        optimizer.step()
        total_it += 1
        with torch.no_grad():
            acc = (torch.argmax(pred_cls, dim=1) == cls_labels).float().mean()
        _scalar(tb_log, 'train_loss', loss.item(), total_it)
        _scalar(tb_log, 'train_acc', acc, total_it)
        if it % 500 == 0:
            log_print('training epoch %d: it=%d/%d, total_it=%d, loss=%.5f, acc=%.3f, lr=%.5f' %
                      (epoch, it, len(train_loader), total_it, loss.item(), acc, lr_scheduler.get_last_lr()[0]), log_f=log_f)
    return total_it


def eval_one_epoch(model, eval_loader, epoch, tb_log=None, log_f=None):
    """train.py:86-118 -> the mean of the batches' accuracies (nan without a batch)."""
    model.eval()
    log_print('===============EVAL EPOCH %d================' % epoch, log_f=log_f)
    acc_list, loss_list = [], []
    for it, batch in enumerate(eval_loader):
        pts_input, cls_labels = _to_device(batch)
        pred_cls = model(pts_input)
        loss_list.append(F.cross_entropy(pred_cls, cls_labels).item())
        acc = (torch.argmax(pred_cls, dim=1) == cls_labels).float().mean()
        acc_list.append(acc.item())
        if it % 100 == 0:
            log_print('EVAL: it=%d/%d, acc=%.3f' % (it, len(eval_loader), acc), log_f=log_f)
    avg_acc = float(np.mean(acc_list)) if acc_list else float('nan')
    avg_loss = float(np.mean(loss_list)) if loss_list else float('nan')
    _scalar(tb_log, 'eval_acc', avg_acc, epoch)
    _scalar(tb_log, 'eval_loss', avg_loss, epoch)
    log_print('\nEpoch %d: Average acc (samples=%d): %.6f' % (epoch, len(acc_list), avg_acc), log_f=log_f)
    return avg_acc


def test_one_epoch(model, test_loader, epoch, log_f=None, labels=None):
    """train.py:120-168 -> (confusion matrix in per cent of each true class, classification report text).  labels: the category
    names in class order (the reference reads them from object_names.txt); None: the test loader's dataset's ``labels`` if it has
    them, else the class indices."""
    from sklearn.metrics import classification_report, confusion_matrix

    model.eval()
    log_print('===============TEST EPOCH %d================' % epoch, log_f=log_f)
    y_truths, y_preds = [], []
    for batch in test_loader:
        y_truths.append(batch[1].numpy().reshape(-1))
        pts_input, _ = _to_device(batch)
        y_preds.append(torch.argmax(model(pts_input), dim=1).cpu().numpy())
    y_truth, y_pred = np.hstack(y_truths), np.hstack(y_preds)
    if labels is None:
        labels = getattr(getattr(test_loader, 'dataset', None), 'labels', None)
    classes = list(range(len(labels))) if labels is not None else None
    conf_mat = confusion_matrix(y_truth, y_pred, labels=classes).astype(np.float64)
    rows = conf_mat.sum(axis=1, keepdims=True)
    conf_mat = 100.0 * np.divide(conf_mat, rows, out=np.zeros_like(conf_mat), where=rows > 0)
    report = classification_report(y_truth, y_pred, labels=classes, target_names=labels, zero_division=0)
    log_print(report, log_f)
    return conf_mat, report


def save_checkpoint(model, epoch, ckpt_name):
    """train.py:171-180: ``<ckpt_name>.pth`` holding {'epoch', 'model_state'}."""
    model_state = model.module.state_dict() if isinstance(model, torch.nn.DataParallel) else model.state_dict()
    ckpt_name = '{}.pth'.format(ckpt_name)
    torch.save({'epoch': epoch, 'model_state': model_state}, ckpt_name)
    log_print(f"save checkpoint to {ckpt_name}")


def load_checkpoint(model, filename):
    """train.py:183-193 -> the checkpoint's epoch.  The tensors are loaded onto the CPU and copied into the model where it is."""
    if not os.path.isfile(filename):
        raise FileNotFoundError(filename)
    log_print("==> Loading from checkpoint %s" % filename)
    checkpoint = torch.load(filename, map_location='cpu')
    model.load_state_dict(checkpoint['model_state'])
    log_print("==> Done")
    return checkpoint['epoch']


def train_and_eval(model, train_loader, eval_loader, tb_log, ckpt_dir, log_f, config, fixed_order=True):
    """train.py:196-219.  config: lr, weight_decay, epochs, ckpt_save_interval, resume ('true' loads config.ckpt and goes on behind
    its epoch).  As in the reference the first epoch is number 2 (``range(start_epoch + 1, epochs + 1)`` from start_epoch = 1) and
    runs at the full ``lr``; the epoch behind k scheduler steps runs at ``lr / (k + 1)``.  Returns the optimizer's learning rate seen
    by every epoch, ``{epoch: lr}``.  fixed_order: as in ``train_one_epoch``, it overrides the global switch for the training steps."""
    model.cuda()
    total_it = 0
    optimizer = torch.optim.Adam(model.parameters(), lr=config.lr, weight_decay=config.weight_decay)
    lr_scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda epoch: 1 / (epoch + 1))
    start_epoch = 1
    if config.resume == 'true':
        start_epoch = load_checkpoint(model, config.ckpt)
    seen = {}
    for epoch in range(start_epoch + 1, config.epochs + 1):
        seen[epoch] = optimizer.param_groups[0]['lr']
        total_it = train_one_epoch(model, train_loader, optimizer, lr_scheduler, epoch, total_it, tb_log, log_f, fixed_order=fixed_order)
        lr_scheduler.step()
        if epoch % config.ckpt_save_interval == 0:
            with torch.no_grad():
                eval_one_epoch(model, eval_loader, epoch, tb_log, log_f)
                save_checkpoint(model, epoch, os.path.join(ckpt_dir, 'checkpoint_epoch_%d' % epoch))
    return seen


def build_parser():
    """train.py:22-40."""
    parser = argparse.ArgumentParser(description="Arg parser")
    parser.add_argument("--batch_size", type=int, default=8)
    parser.add_argument("--epochs", type=int, default=100)
    parser.add_argument("--ckpt_save_interval", type=int, default=5)
    parser.add_argument('--workers', type=int, default=4)
    parser.add_argument("--mode", type=str, default='train')
    parser.add_argument("--ckpt", type=str, default='None')
    parser.add_argument("--net", type=str, default='pointnet2_msg_cls')
    parser.add_argument('--lr', type=float, default=0.003)
    parser.add_argument('--lr_decay', type=float, default=0.7)
    parser.add_argument('--weight_decay', type=float, default=0.0)
    parser.add_argument("--output_dir", type=str, default='./output')
    parser.add_argument("--extra_tag", type=str, default='default')
    parser.add_argument("--resume", type=str, default='false')
    parser.add_argument("--data_root", type=str, default='./data/resampled_KITTI')     # (a constant in the reference)
    return parser


def main(argv=None):
    """train.py:222-265: modes train, eval and test over ``--data_root``."""
    args = build_parser().parse_args(argv)
    nets = {'pointnet2_msg_cls': PointNet2ClassificationMSG, 'pointnet2_ssg_cls': PointNet2ClassificationSSG}
    if args.net not in nets:
        raise NotImplementedError(args.net)
    model = nets[args.net]()
    train_loader, valid_loader, test_loader = KITTIPCDClsDataset_Wrapper(args.data_root, args).get_dataloader()
    if args.mode == 'train':
        output_dir = os.path.join(args.output_dir, args.extra_tag)
        ckpt_dir = os.path.join(output_dir, 'ckpt')
        os.makedirs(ckpt_dir, exist_ok=True)
        with open(os.path.join(output_dir, 'log.txt'), 'w') as log_f:
            for key, val in vars(args).items():
                log_print("{:16} {}".format(key, val), log_f=log_f)
            train_and_eval(model, train_loader, valid_loader, None, ckpt_dir, log_f, args)
    elif args.mode == 'eval':
        epoch = load_checkpoint(model, args.ckpt)
        model.cuda()
        with torch.no_grad():
            eval_one_epoch(model, valid_loader, epoch)
    elif args.mode == 'test':
        output_test_dir = os.path.join(args.output_dir, args.extra_tag, 'test')
        os.makedirs(output_test_dir, exist_ok=True)
        with open(os.path.join(output_test_dir, 'log.txt'), 'w') as log_f:
            epoch = load_checkpoint(model, args.ckpt)
            model.cuda()
            with torch.no_grad():
                test_one_epoch(model, test_loader, epoch, log_f)
    else:
        raise NotImplementedError(args.mode)


if __name__ == '__main__':
    main()
