"""CPU tests of utils/run_train_rounds.py's supervision of its children, with stand-in children that sleep: SIGTERM to
the driver stops the running training child or labelling workers before the driver exits, and a driver killed
outright (SIGKILL) takes them with it through the parent-death signal.  Also: the training rounds' validation shape is
--val_eval_shape, not the labelling --eval_shape."""
import importlib
import os
import signal
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
rtr = importlib.import_module('utils.run_train_rounds')

pytestmark = pytest.mark.skipif(not os.path.isdir('/proc/self'), reason='reads the process table from /proc')

_TRAINING = r'''
import importlib, sys
sys.path.insert(0, sys.argv[1])
rtr = importlib.import_module('utils.run_train_rounds')
rtr.install_signal_handlers()
try:
    rtr.run_training([sys.executable, '-c', 'import time; time.sleep(600)  # stand-in training child'], 0)
except rtr.Interrupted as e:
    sys.exit(128 + e.signum)
'''

_WORKERS = r'''
import importlib, sys, time
sys.path.insert(0, sys.argv[1])
rtr = importlib.import_module('utils.run_train_rounds')
rtr.install_signal_handlers()
try:
    rtr.run_workers(time.sleep, [600, 600], 0)
except rtr.Interrupted as e:
    sys.exit(128 + e.signum)
'''


def _state(pid):
    """the process state letter, or None when there is no such process"""
    try:
        with open('/proc/%d/stat' % pid) as fp:
            stat = fp.read()
    except OSError:
        return None
    return stat[stat.rindex(')') + 2:].split()[0]


def _alive(pid):
    return _state(pid) not in (None, 'Z', 'X')


def _children(pid, mark):
    out = []
    for d in os.listdir('/proc'):
        if not d.isdigit():
            continue
        try:
            with open('/proc/%s/stat' % d) as fp:
                stat = fp.read()
            with open('/proc/%s/cmdline' % d, 'rb') as fp:
                cmd = fp.read().decode(errors='replace')
        except OSError:
            continue
        fields = stat[stat.rindex(')') + 2:].split()
        if int(fields[1]) == pid and mark in cmd and fields[0] not in ('Z', 'X'):
            out.append(int(d))
    return out


def _wait_for(cond, secs):
    t = time.time() + secs
    while time.time() < t:
        if cond():
            return True
        time.sleep(0.1)
    return cond()


def _start(script, mark, n):
    drv = subprocess.Popen([sys.executable, '-c', script, ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    kids = []
    try:
        assert _wait_for(lambda: len(_children(drv.pid, mark)) == n, 60), drv.pid
        kids = _children(drv.pid, mark)
    except BaseException:
        drv.kill()
        drv.wait()
        raise
    return drv, kids


def _finish(drv, kids, sig):
    try:
        os.kill(drv.pid, sig)
        out = drv.communicate(timeout=120)[0].decode()
        gone = _wait_for(lambda: not any(_alive(k) for k in kids), 30)
    finally:
        for k in kids:
            if _alive(k):
                os.kill(k, signal.SIGKILL)
        if drv.poll() is None:
            drv.kill()
            drv.wait()
    assert gone, 'a child outlived the driver: ' + out[-2000:]
    return drv.returncode, out


@pytest.mark.parametrize('sig', [signal.SIGTERM, signal.SIGINT, signal.SIGKILL])
def test_training_child_does_not_outlive_the_driver(sig):
    drv, kids = _start(_TRAINING, 'stand-in training child', 1)
    rc, out = _finish(drv, kids, sig)
    assert rc == (-9 if sig == signal.SIGKILL else 128 + sig), out[-2000:]


@pytest.mark.parametrize('sig', [signal.SIGTERM, signal.SIGKILL])
def test_labelling_workers_do_not_outlive_the_driver(sig):
    drv, kids = _start(_WORKERS, 'spawn_main', 2)
    rc, out = _finish(drv, kids, sig)
    assert rc == (-9 if sig == signal.SIGKILL else 128 + sig), out[-2000:]


def test_failing_worker_stops_its_siblings():
    t0 = time.time()
    with pytest.raises(rtr.ChildFailed, match='exited with status 1'):
        rtr.run_workers(sys.exit, [1, 0], 0)
    with pytest.raises(rtr.ChildFailed, match='timed out'):
        rtr.run_workers(time.sleep, [600], 2)
    assert time.time() - t0 < 120


def test_training_validation_shape_is_its_own():
    a = rtr.get_args(['--eval_shape', '512', '1024'])
    argv = rtr.train_argv(a, rtr.plan(a, 'F')[0], 'D1', {})
    i = argv.index('--eval_shape')
    assert argv[i + 1:i + 3] == ['1024', '2048'] and argv.count('--eval_shape') == 1
    b = rtr.get_args(['--val_eval_shape', '64', '128'])
    argv = rtr.train_argv(b, rtr.plan(b, 'F')[0], 'D1', {})
    i = argv.index('--eval_shape')
    assert argv[i + 1:i + 3] == ['64', '128']
