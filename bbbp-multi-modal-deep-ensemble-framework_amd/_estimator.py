"""``get_params`` / ``set_params`` for the estimators that ``ensemble`` clones: one form for all of them, ``naive_bayes.BernoulliNB``'s."""


class Params:
    """A class lists its constructor's parameters in ``_params`` and keeps each under its own name.  ``set_params`` passes the whole set, the
    changes included, through the constructor's checks before anything is stored, and stores what the constructor made of each value."""

    _params = ()

    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in self._params}

    def set_params(self, **params):
        unknown = set(params) - set(self._params)
        if unknown:
            raise ValueError(f"{type(self).__name__}: unknown parameters {sorted(unknown)}")
        checked = type(self)(**{**self.get_params(), **params})          # the constructor's checks
        for name in params:
            setattr(self, name, getattr(checked, name))
        return self
